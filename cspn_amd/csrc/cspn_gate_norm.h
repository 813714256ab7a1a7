// cspn_gate_norm.h -- the demo's gate normalisation (reference cspn_paddle/demo.py:24,34-36,47-49: abs, reduce_sum over the K gate
// channels of a slice, elementwise_div) in ONE arithmetic form, shared by the stand-alone normaliser (cspn_gate_norm.hip) and the fused
// persistent 3D instance (cspn3d_persistent.hip, NRM): both compute w_k = |g_k| * r with r = 1 / S, S = sum_{j=0..K-1} |g_j| added in
// channel order, so the fused and the unfused path agree bit for bit.  IEEE division: an all-zero voxel gives r = inf and
// w = 0 * inf = NaN, where torch's 0 / 0 gives NaN.
#pragma once
#include <hip/hip_runtime.h>

namespace cspn {

// g(k) returns gate k of the voxel (k = 0 .. K-1)
template <int K, class G>
__device__ __forceinline__ float absnorm_rcp(G g) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) s += fabsf(g(k));
    return 1.f / s;
}

__device__ __forceinline__ float absnorm_gate(float g, float r) { return fabsf(g) * r; }

}  // namespace cspn
