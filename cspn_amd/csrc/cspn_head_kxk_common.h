// cspn_head_kxk_common.h -- what the float32 and the 16-bit heads for K x K propagation (cspn_head_kxk.hip, cspn_head_kxk_g16.hip) share: the waves' units
// of work, and of dL/dW the sizes, the launch geometry and the sum over the workgroups.
#pragma once
#include "cspn_common.h"

namespace cspn {

typedef float f16v __attribute__((ext_vector_type(16)));

// a wave's unit of work: workgroup ids go round the 8 XCDs, each XCD takes a contiguous eighth of the units (neighbouring rows share a row of their input in one L2)
__device__ __forceinline__ int wave_unit() {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per_xcd = gridDim.x >> 3;
    return (((int)blockIdx.x & 7) * per_xcd + ((int)blockIdx.x >> 3)) * 4 + wv;
}

// waves -> workgroups, a multiple of 8 (wave_unit's XCD mapping; the spare waves return at once); 0: does not fit an int
inline unsigned groups_of(long long units) {
    const long long groups = ((units + 3) / 4 + 7) / 8 * 8;
    return groups * 4 >= (1ll << 31) ? 0u : (unsigned)groups;      // (the kernels number the waves with an int)
}

// ---- dL/dW: D[row T = o * 9 + r * 3 + k][channel], rows in blocks of 32, blockIdx.y = a group of DW_TB row blocks, NB blocks of 32 channels ----
constexpr int DW_TB = 4;
constexpr int DW_MAX_WG = 256;        // workgroups per group of row blocks (one per CU)
template <int NB>
struct DwSize { static constexpr int floats = DW_TB * NB * 16 * 64; };   // a workgroup's partial block

inline int row_groups(int O) { return ((9 * O + 31) / 32 + DW_TB - 1) / DW_TB; }

// the launch geometry: tiles of tile_px consecutive pixels of the fed input rows, shared out among nwave waves of nwg workgroups, ng groups of row blocks
struct DwGeo {
    int hfed, tiles_w, tiles, nwave, nwg, ng;
    bool fits;       // false: more tiles than an int counts
    DwGeo(int B, int h, int w, int H, int W, int O, int tile_px) {
        hfed = (H + 1) / 2 < h ? (H + 1) / 2 : h;     // input rows whose unpooled row lies inside the (narrowed) output
        const int wfed = (W + 1) / 2 < w ? (W + 1) / 2 : w;
        tiles_w = (wfed + tile_px - 1) / tile_px;
        const long long tiles_ll = (long long)B * hfed * tiles_w;
        fits = tiles_ll < (1ll << 31);
        tiles = fits ? (int)tiles_ll : 0;
        nwave = tiles < 4 * DW_MAX_WG ? tiles : 4 * DW_MAX_WG;
        nwg = (nwave + 3) / 4;
        ng = row_groups(O);
    }
};

// dW[o][c][ky][kx] of channels c0 .. c0 + 32 NB - 1 = the sum of the nwg workgroups' blocks in part, in workgroup order (cspn_head_kxk.hip)
void head_kxk_dw_reduce(const float* part, float* dwg, float* dwb, int C, int c0, int NB, int O, int nwg, hipStream_t st);

}  // namespace cspn
