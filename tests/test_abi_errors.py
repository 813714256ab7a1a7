"""CPU: every host-side argument check of the 3 x 3 entry points in 2D and 3D (and the size queries next to them), pinned row by row: the
return code and the full cspn_last_error() text.  The pointers are fake, so every row ends in a host-side return before any copy or
launch (a size rule may ask the runtime for the device's compute-unit count; with no device it takes its default).  Where the text
carries the workspace's byte count, which may depend on that count, the row pins the code and the text up to the number.  The library
is called through a handle of this test's own with explicitly typed arguments: the C ABI is what is pinned, not the Python binding."""
import ctypes

import pytest

from cspn_amd import _lib


class P(object):
    """a pointer argument: None or a fake address"""
    def __init__(self, v):
        self.v = v


class Z(P):
    """a size_t argument"""


def _c(a):
    if isinstance(a, Z):
        return ctypes.c_size_t(a.v)
    if isinstance(a, P):
        return ctypes.c_void_p(a.v)
    return ctypes.c_int(a)


# queries that return a size_t; everything else returns an int
_SIZE_T = {"cspn2d_workspace_bytes", "cspn2d_backward_workspace_bytes", "cspn2d_history_bytes", "cspn2d_backward_history_workspace_bytes",
           "cspn2d_workspace_bytes_multi", "cspn2d_backward_multi_workspace_bytes", "cspn2d_history_bytes_multi",
           "cspn2d_backward_history_multi_workspace_bytes", "cspn3d_workspace_bytes", "cspn3d_workspace_bytes_ex",
           "cspn3d_backward_workspace_bytes", "cspn3d_backward_multi_workspace_bytes", "cspn3d_forward_absnorm_workspace_bytes"}

# (symbol, the check the row reaches, arguments, return value, cspn_last_error() text).  Text None: the call returns 0 and writes none.
# A text that ends in "need " is compared up to there (the byte count behind it may depend on the device).
ROWS = [
    ('cspn2d_forward_f32_algo', 'bad shape', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 0, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 H=0 W=4'),
    ('cspn2d_forward_f32_algo', 'B == 0', (P(0x10000), P(0x20000), P(None), P(0x40000), 0, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn2d_forward_f32_algo', 'too large for 32-bit indexing', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 20000, 20000, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing'),
    ('cspn2d_forward_f32_algo', 'padded path refused', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 8, 3, 0, 4, P(0x90000), Z(0x10000000000), P(None)), -3, 'FUSED_PADDED needs W % 4 != 0 and a shape the fused kernels take (B=1 H=4 W=8 n_iter=3)'),
    ('cspn2d_forward_f32_algo', 'padded path, workspace not 16-byte aligned', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 5, 3, 0, 4, P(0x90004), Z(0x10000000000), P(None)), -3, 'FUSED_PADDED needs a 16-byte aligned workspace (its padded planes live there)'),
    ('cspn2d_forward_f32_algo', 'padded path, null pointer', (P(None), P(0x20000), P(None), P(0x40000), 1, 4, 5, 3, 0, 4, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_forward_f32_algo', 'padded path, workspace too small', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 5, 3, 0, 4, P(0x90000), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_forward_f32_algo', 'unknown algo', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 4, 3, 0, 9, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown algo 9'),
    ('cspn2d_forward_f32_algo', 'fused refused', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 5, 3, 0, 2, P(0x90000), Z(0x10000000000), P(None)), -3, 'fused kernel does not support B=1 H=4 W=5 n_iter=3'),
    ('cspn2d_forward_f32_algo', 'null pointer', (P(None), P(0x20000), P(None), P(0x40000), 1, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_forward_f32_algo', 'null pointer (out)', (P(0x10000), P(0x20000), P(None), P(None), 1, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_forward_f32_algo', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 4, -1, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'n_iter must be >= 0 (got -1)'),
    ('cspn2d_forward_f32_algo', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 4, 3, 7, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type 7'),
    ('cspn2d_forward_f32_algo', 'workspace too small', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 4, 3, 0, 1, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_forward_f32_algo', 'workspace too small (bytes)', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 4, 3, 0, 1, P(0x90000), Z(16), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_forward_f32_algo', 'workspace misaligned', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 4, 3, 0, 1, P(0x90010), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn2d_forward_f32_algo', 'auto on W % 4 != 0, workspace too small', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 4, 5, 3, 0, 0, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_backward_f32', 'bad shape', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 4, -1, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 H=4 W=-1'),
    ('cspn2d_backward_f32', 'B == 0', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 0, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn2d_backward_f32', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 4, 4, 0, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'backward needs n_iter >= 1 (got 0)'),
    ('cspn2d_backward_f32', 'too large for 32-bit indexing', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 20000, 20000, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing'),
    ('cspn2d_backward_f32', 'missing grad_out', (P(0x10000), P(0x20000), P(None), P(None), P(0x60000), P(0x70000), 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null grad_out'),
    ('cspn2d_backward_f32', 'null pointer', (P(0x10000), P(None), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_backward_f32', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 4, 4, 3, -1, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type -1'),
    ('cspn2d_backward_f32', 'workspace too small', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 4, 4, 3, 0, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_backward_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 4, 4, 3, 0, P(0x90080), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn2d_backward_f32', 'both gradients null', (P(0x10000), P(0x20000), P(None), P(0x50000), P(None), P(None), 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn2d_forward_history_f32', 'bad shape (B == 0)', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 0, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=0 H=64 W=512'),
    ('cspn2d_forward_history_f32', 'bad shape', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 2, 0, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=2 H=0 W=512'),
    ('cspn2d_forward_history_f32', 'no history mode', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'no history mode for B=1 H=4 W=4 n_iter=3'),
    ('cspn2d_forward_history_f32', 'no history mode (n_iter)', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 2, 64, 512, -1, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'no history mode for B=2 H=64 W=512 n_iter=-1'),
    ('cspn2d_forward_history_f32', 'history missing', (P(0x10000), P(0x20000), P(None), P(0x40000), P(None), Z(0x10000000000), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -2, 'history buffer too small or misaligned: need 3473408 bytes'),
    ('cspn2d_forward_history_f32', 'history too small', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(256), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -2, 'history buffer too small or misaligned: need 3473408 bytes'),
    ('cspn2d_forward_history_f32', 'history misaligned', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80010), Z(0x10000000000), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -2, 'history buffer too small or misaligned: need 3473408 bytes'),
    ('cspn2d_forward_history_f32', 'null pointer', (P(None), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_forward_history_f32', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 2, 64, 512, 24, 4, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type 4'),
    ('cspn2d_forward_history_f32', 'output misaligned', (P(0x10000), P(0x20000), P(None), P(0x40004), P(0x80000), Z(0x10000000000), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'output must be 16-byte aligned'),
    ('cspn2d_backward_history_f32', 'bad shape (B == 0)', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 0, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=0 H=64 W=512'),
    ('cspn2d_backward_history_f32', 'no history mode', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'no history mode for B=1 H=4 W=4 n_iter=3'),
    ('cspn2d_backward_history_f32', 'missing grad_out', (P(0x10000), P(0x20000), P(None), P(None), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null grad_out'),
    ('cspn2d_backward_history_f32', 'history missing', (P(0x10000), P(0x20000), P(None), P(0x50000), P(None), Z(0x10000000000), P(0x60000), P(0x70000), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -2, 'history buffer too small: need 3473408 bytes'),
    ('cspn2d_backward_history_f32', 'history too small', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(256), P(0x60000), P(0x70000), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -2, 'history buffer too small: need 3473408 bytes'),
    ('cspn2d_backward_history_f32', 'null pointer', (P(None), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_backward_history_f32', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 64, 512, 24, 9, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type 9'),
    ('cspn2d_backward_history_f32', 'workspace too small', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 64, 512, 24, 0, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_backward_history_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 64, 512, 24, 0, P(0x90040), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn2d_backward_history_f32', 'both gradients null', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(None), P(None), 2, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn2d_forward_multi_f32', 'bad shape', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 0, 1, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 C=0 H=4 W=4'),
    ('cspn2d_forward_multi_f32', 'bad shape (B < 0)', (P(0x10000), P(0x20000), P(None), P(0x40000), -1, 2, 1, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=-1 C=2 H=4 W=4'),
    ('cspn2d_forward_multi_f32', 'bad sparse channel count', (P(0x10000), P(0x20000), P(0x30000), P(0x40000), 1, 2, 3, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'sparse has 3 channels: 1 (one mask for every channel) or C = 2 expected'),
    ('cspn2d_forward_multi_f32', 'too large for 32-bit indexing', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 1, 20000, 10000, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing (B*C*H*W)'),
    ('cspn2d_forward_multi_f32', "C == 1: the single-channel entry's error", (P(None), P(0x20000), P(None), P(0x40000), 1, 1, 1, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_forward_multi_f32', "C == 1: the single-channel entry's shape text", (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 1, 1, 20000, 20000, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing (B*C*H*W)'),
    ('cspn2d_forward_multi_f32', 'B == 0', (P(0x10000), P(0x20000), P(None), P(0x40000), 0, 2, 1, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn2d_forward_multi_f32', 'unknown algo', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 1, 4, 4, 3, 0, 5, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown algo 5'),
    ('cspn2d_forward_multi_f32', 'null pointer', (P(0x10000), P(None), P(None), P(0x40000), 1, 2, 1, 4, 4, 3, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_forward_multi_f32', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 1, 4, 4, -2, 0, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'n_iter must be >= 0 (got -2)'),
    ('cspn2d_forward_multi_f32', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 1, 4, 4, 3, 11, 1, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type 11'),
    ('cspn2d_forward_multi_f32', 'workspace too small', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 1, 4, 4, 3, 0, 1, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_forward_multi_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 1, 4, 4, 3, 0, 1, P(0x90020), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn2d_backward_multi_f32', 'bad shape', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 2, 1, 0, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 C=2 H=0 W=4'),
    ('cspn2d_backward_multi_f32', 'bad sparse channel count', (P(0x10000), P(0x20000), P(0x30000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 0, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'sparse has 0 channels: 1 (one mask for every channel) or C = 2 expected'),
    ('cspn2d_backward_multi_f32', 'too large for 32-bit indexing', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 3, 1, 10000, 10000, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing (B*C*H*W)'),
    ('cspn2d_backward_multi_f32', "C == 1: the single-channel entry's error", (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 1, 1, 4, 4, 0, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'backward needs n_iter >= 1 (got 0)'),
    ('cspn2d_backward_multi_f32', 'B == 0', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 0, 2, 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn2d_backward_multi_f32', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 2, 1, 4, 4, 0, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'backward needs n_iter >= 1 (got 0)'),
    ('cspn2d_backward_multi_f32', 'missing grad_out', (P(0x10000), P(0x20000), P(None), P(None), P(0x60000), P(0x70000), 1, 2, 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null grad_out'),
    ('cspn2d_backward_multi_f32', 'null pointer', (P(None), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 2, 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_backward_multi_f32', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 2, 1, 4, 4, 3, 5, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type 5'),
    ('cspn2d_backward_multi_f32', 'workspace too small', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 2, 1, 4, 4, 3, 0, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_backward_multi_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 2, 1, 4, 4, 3, 0, P(0x90008), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn2d_backward_multi_f32', 'both gradients null', (P(0x10000), P(0x20000), P(None), P(0x50000), P(None), P(None), 1, 2, 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn2d_forward_history_multi_f32', 'bad shape', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 2, 2, 1, 64, 0, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=2 C=2 H=64 W=0'),
    ('cspn2d_forward_history_multi_f32', 'bad sparse channel count', (P(0x10000), P(0x20000), P(0x30000), P(0x40000), P(0x80000), Z(0x10000000000), 2, 2, 5, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'sparse has 5 channels: 1 (one mask for every channel) or C = 2 expected'),
    ('cspn2d_forward_history_multi_f32', "C == 1: the single-channel entry's texts", (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 1, 1, 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'no history mode for B=1 H=4 W=4 n_iter=3'),
    ('cspn2d_forward_history_multi_f32', 'C == 1, B == 0', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 0, 1, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=0 H=64 W=512'),
    ('cspn2d_forward_history_multi_f32', 'B == 0', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 0, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=0'),
    ('cspn2d_forward_history_multi_f32', 'no history mode', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 1, 2, 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'no history mode for B=1 C=2 H=4 W=4 n_iter=3'),
    ('cspn2d_forward_history_multi_f32', 'history missing', (P(0x10000), P(0x20000), P(None), P(0x40000), P(None), Z(0x10000000000), 2, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -2, 'history buffer too small or misaligned: need 6881280 bytes'),
    ('cspn2d_forward_history_multi_f32', 'history misaligned', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80080), Z(0x10000000000), 2, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -2, 'history buffer too small or misaligned: need 6881280 bytes'),
    ('cspn2d_forward_history_multi_f32', 'null pointer', (P(0x10000), P(0x20000), P(None), P(None), P(0x80000), Z(0x10000000000), 2, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_forward_history_multi_f32', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 2, 2, 1, 64, 512, 24, -3, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type -3'),
    ('cspn2d_forward_history_multi_f32', 'workspace too small', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 2, 2, 1, 64, 512, 24, 0, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_forward_history_multi_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(None), P(0x40000), P(0x80000), Z(0x10000000000), 2, 2, 1, 64, 512, 24, 0, P(0x90010), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn2d_forward_history_multi_f32', 'output misaligned', (P(0x10000), P(0x20000), P(None), P(0x40008), P(0x80000), Z(0x10000000000), 2, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'output must be 16-byte aligned'),
    ('cspn2d_backward_history_multi_f32', 'bad shape', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, -1, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=2 C=-1 H=64 W=512'),
    ('cspn2d_backward_history_multi_f32', 'bad sparse channel count', (P(0x10000), P(0x20000), P(0x30000), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 2, 3, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'sparse has 3 channels: 1 (one mask for every channel) or C = 2 expected'),
    ('cspn2d_backward_history_multi_f32', "C == 1: the single-channel entry's texts", (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 1, 1, 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'no history mode for B=1 H=4 W=4 n_iter=3'),
    ('cspn2d_backward_history_multi_f32', 'B == 0', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 0, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=0'),
    ('cspn2d_backward_history_multi_f32', 'no history mode', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 1, 2, 1, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'no history mode for B=1 C=2 H=4 W=4 n_iter=3'),
    ('cspn2d_backward_history_multi_f32', 'missing grad_out', (P(0x10000), P(0x20000), P(None), P(None), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null grad_out'),
    ('cspn2d_backward_history_multi_f32', 'history too small', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(1024), P(0x60000), P(0x70000), 2, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -2, 'history buffer too small: need 6881280 bytes'),
    ('cspn2d_backward_history_multi_f32', 'null pointer', (P(0x10000), P(None), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn2d_backward_history_multi_f32', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 2, 1, 64, 512, 24, 6, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type 6'),
    ('cspn2d_backward_history_multi_f32', 'workspace too small', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 2, 1, 64, 512, 24, 0, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn2d_backward_history_multi_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(0x60000), P(0x70000), 2, 2, 1, 64, 512, 24, 0, P(0x90004), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn2d_backward_history_multi_f32', 'both gradients null', (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x80000), Z(0x10000000000), P(None), P(None), 2, 2, 1, 64, 512, 24, 0, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn3d_forward_f32_algo', 'bad shape', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 0, 4, 4, 3, 2, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 D=0 H=4 W=4'),
    ('cspn3d_forward_f32_algo', 'B == 0', (P(0x10000), P(0x20000), P(None), P(0x40000), 0, 2, 4, 4, 3, 2, 0, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn3d_forward_f32_algo', 'too large for 32-bit indexing', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 1000, 1000, 100, 3, 2, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing'),
    ('cspn3d_forward_f32_algo', 'unknown algo', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 4, 4, 3, 2, 3, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown 3D algo 3'),
    ('cspn3d_forward_f32_algo', 'null pointer', (P(None), P(0x20000), P(None), P(0x40000), 1, 2, 4, 4, 3, 2, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn3d_forward_f32_algo', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 4, 4, -1, 2, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'n_iter must be >= 0 (got -1)'),
    ('cspn3d_forward_f32_algo', 'unknown norm', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 4, 4, 3, 7, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown norm_type 7'),
    ('cspn3d_forward_f32_algo', 'prenorm refused in 3D', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 4, 4, 3, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'norm_type CSPN_NORM_PRENORM is taken by the 2D entry points only'),
    ('cspn3d_forward_f32_algo', 'workspace too small', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 4, 4, 3, 2, 0, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn3d_forward_f32_algo', 'workspace too small (normalising mode)', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 4, 4, 3, 0, 0, P(0x90000), Z(64), P(None)), -2, 'workspace too small: need '),
    ('cspn3d_forward_f32_algo', 'workspace misaligned', (P(0x10000), P(0x20000), P(None), P(0x40000), 1, 2, 4, 4, 3, 2, 0, P(0x90010), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn3d_forward_multi_f32', 'bad shape', (P(0x10000), P(0x20000), P(0x40000), 1, 0, 2, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 C=0 D=2 H=4 W=4'),
    ('cspn3d_forward_multi_f32', 'B == 0', (P(0x10000), P(0x20000), P(0x40000), 0, 2, 2, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn3d_forward_multi_f32', 'null pointer', (P(0x10000), P(None), P(0x40000), 1, 2, 2, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn3d_forward_multi_f32', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 2, 4, 4, -1, P(0x90000), Z(0x10000000000), P(None)), -1, 'n_iter must be >= 0 (got -1)'),
    ('cspn3d_forward_multi_f32', 'workspace too small', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 2, 4, 4, 3, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn3d_forward_multi_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 2, 4, 4, 3, P(0x90010), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn3d_forward_multi_f32', 'persistent kernel only', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 2, 4, 4, 1, P(0x90000), Z(0x10000000000), P(None)), -3, 'cspn3d_forward_multi_f32 runs the persistent kernel only (W % 4 == 0, 2 <= n_iter <= 60, 16-byte aligned tensors, volume resident on the device): loop over the channels with cspn3d_forward_f32 for B=1 C=2 D=2 H=4 W=4 n_iter=1'),
    ('cspn3d_forward_multi_f32', 'persistent kernel only (W % 4)', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 2, 4, 5, 3, P(0x90000), Z(0x10000000000), P(None)), -3, 'cspn3d_forward_multi_f32 runs the persistent kernel only (W % 4 == 0, 2 <= n_iter <= 60, 16-byte aligned tensors, volume resident on the device): loop over the channels with cspn3d_forward_f32 for B=1 C=2 D=2 H=4 W=5 n_iter=3'),
    ('cspn3d_backward_f32', 'bad shape', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 4, 0, 3, 2, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 D=2 H=4 W=0'),
    ('cspn3d_backward_f32', 'B == 0', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 0, 2, 4, 4, 3, 2, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn3d_backward_f32', 'too large for 32-bit indexing', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 1000, 1000, 100, 3, 2, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing'),
    ('cspn3d_backward_f32', 'non-NONE norm', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'the 3D backward covers the Paddle contract only (norm_type NONE: gates used as given, no mask)'),
    ('cspn3d_backward_f32', 'non-NONE norm (prenorm)', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 4, 4, 3, 3, P(0x90000), Z(0x10000000000), P(None)), -3, 'the 3D backward covers the Paddle contract only (norm_type NONE: gates used as given, no mask)'),
    ('cspn3d_backward_f32', 'null pointer', (P(None), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 4, 4, 3, 2, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn3d_backward_f32', 'missing grad_out', (P(0x10000), P(0x20000), P(None), P(0x60000), P(0x70000), 1, 2, 4, 4, 3, 2, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn3d_backward_f32', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 4, 4, -1, 2, P(0x90000), Z(0x10000000000), P(None)), -1, 'n_iter must be >= 0 (got -1)'),
    ('cspn3d_backward_f32', 'workspace too small', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 4, 4, 3, 2, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn3d_backward_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 4, 4, 3, 2, P(0x90010), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn3d_backward_f32', 'both gradients null', (P(0x10000), P(0x20000), P(0x50000), P(None), P(None), 1, 2, 4, 4, 3, 2, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn3d_backward_f32', 'both gradients null, n_iter == 0', (P(0x10000), P(0x20000), P(0x50000), P(None), P(None), 1, 2, 4, 4, 0, 2, P(None), Z(0), P(None)), 0, None),
    ('cspn3d_backward_multi_f32', 'bad shape', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 0, 2, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 C=0 D=2 H=4 W=4'),
    ('cspn3d_backward_multi_f32', 'bad shape (D)', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, -4, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 C=2 D=-4 H=4 W=4'),
    ('cspn3d_backward_multi_f32', 'B == 0', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 0, 2, 2, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn3d_backward_multi_f32', 'too large for 32-bit indexing (gates)', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 1000, 1000, 100, 3, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing'),
    ('cspn3d_backward_multi_f32', 'too large for 32-bit indexing (values)', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 200, 100, 1000, 100, 3, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing'),
    ('cspn3d_backward_multi_f32', 'null pointer', (P(0x10000), P(None), P(0x50000), P(0x60000), P(0x70000), 1, 2, 2, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn3d_backward_multi_f32', 'missing grad_out', (P(0x10000), P(0x20000), P(None), P(0x60000), P(0x70000), 1, 2, 2, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn3d_backward_multi_f32', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 2, 4, 4, -1, P(0x90000), Z(0x10000000000), P(None)), -1, 'n_iter must be >= 0 (got -1)'),
    ('cspn3d_backward_multi_f32', 'workspace too small', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 2, 4, 4, 3, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn3d_backward_multi_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), 1, 2, 2, 4, 4, 3, P(0x90010), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn3d_backward_multi_f32', 'both gradients null', (P(0x10000), P(0x20000), P(0x50000), P(None), P(None), 1, 2, 2, 4, 4, 3, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn3d_backward_multi_f32', 'both gradients null, n_iter == 0', (P(0x10000), P(0x20000), P(0x50000), P(None), P(None), 1, 2, 2, 4, 4, 0, P(None), Z(0), P(None)), 0, None),
    ('cspn3d_forward_absnorm_f32', 'bad shape', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 0, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'bad shape B=1 D=2 H=0 W=4'),
    ('cspn3d_forward_absnorm_f32', 'B == 0', (P(0x10000), P(0x20000), P(0x40000), 0, 2, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), 0, None),
    ('cspn3d_forward_absnorm_f32', 'too large for 32-bit indexing', (P(0x10000), P(0x20000), P(0x40000), 1, 1000, 1000, 100, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -3, 'tensor too large for 32-bit plane indexing'),
    ('cspn3d_forward_absnorm_f32', 'unknown algo', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 4, 4, 3, -1, P(0x90000), Z(0x10000000000), P(None)), -1, 'unknown 3D algo -1'),
    ('cspn3d_forward_absnorm_f32', 'out aliases feat', (P(0x10000), P(0x20000), P(0x20000), 1, 2, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'cspn3d_forward_absnorm_f32: out must not alias an input'),
    ('cspn3d_forward_absnorm_f32', 'out aliases guide', (P(0x10000), P(0x20000), P(0x10040), 1, 2, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'cspn3d_forward_absnorm_f32: out must not alias an input'),
    ('cspn3d_forward_absnorm_f32', 'null pointer', (P(None), P(0x20000), P(0x40000), 1, 2, 4, 4, 3, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'null tensor pointer'),
    ('cspn3d_forward_absnorm_f32', 'n_iter below the minimum', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 4, 4, -1, 0, P(0x90000), Z(0x10000000000), P(None)), -1, 'n_iter must be >= 0 (got -1)'),
    ('cspn3d_forward_absnorm_f32', 'workspace too small', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 4, 4, 3, 0, P(None), Z(0), P(None)), -2, 'workspace too small: need '),
    ('cspn3d_forward_absnorm_f32', 'workspace misaligned', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 4, 4, 3, 0, P(0x90010), Z(0x10000000000), P(None)), -2, 'workspace must be 256-byte aligned'),
    ('cspn3d_forward_absnorm_f32', 'persistent refused', (P(0x10000), P(0x20000), P(0x40000), 1, 2, 4, 4, 1, 2, P(0x90000), Z(0x10000000000), P(None)), -3, 'persistent 3D kernel does not take this call (needs W % 4 == 0, 16-byte aligned tensors, 2 <= n_iter <= 60, a chunk per device)'),
    ('cspn2d_workspace_bytes', 'bad shape', (0, 4, 4, 3), 0, None),
    ('cspn2d_workspace_bytes', 'n_iter == 0', (1, 4, 4, 0), 0, None),
    ('cspn2d_backward_workspace_bytes', 'bad shape', (0, 4, 4, 3), 0, None),
    ('cspn2d_backward_workspace_bytes', 'n_iter == 0', (1, 4, 4, 0), 0, None),
    ('cspn2d_history_bytes', 'bad shape', (1, 0, 4, 24), 0, None),
    ('cspn2d_history_bytes', 'no history mode', (1, 4, 4, 3), 0, None),
    ('cspn2d_history_bytes', 'no history mode (small image)', (1, 17, 30, 24), 0, None),
    ('cspn2d_backward_history_workspace_bytes', 'bad shape', (1, 0, 4, 24), 0, None),
    ('cspn2d_backward_history_workspace_bytes', 'no history mode', (1, 4, 4, 3), 0, None),
    ('cspn2d_backward_history_workspace_bytes', 'no history mode (small image)', (1, 17, 30, 24), 0, None),
    ('cspn2d_workspace_bytes_multi', 'bad shape', (1, 0, 4, 4, 3), 0, None),
    ('cspn2d_workspace_bytes_multi', 'n_iter == 0', (1, 2, 4, 4, 0), 0, None),
    ('cspn2d_backward_multi_workspace_bytes', 'bad shape', (1, 0, 4, 4, 3), 0, None),
    ('cspn2d_backward_multi_workspace_bytes', 'n_iter == 0', (1, 2, 4, 4, 0), 0, None),
    ('cspn2d_history_bytes_multi', 'bad shape', (1, -1, 4, 4, 24), 0, None),
    ('cspn2d_history_bytes_multi', 'no history mode', (1, 2, 4, 4, 3), 0, None),
    ('cspn2d_history_bytes_multi', 'no history mode (small image)', (1, 2, 17, 30, 24), 0, None),
    ('cspn2d_history_bytes_multi', 'C == 1, no history mode', (1, 1, 17, 30, 24), 0, None),
    ('cspn2d_backward_history_multi_workspace_bytes', 'bad shape', (1, -1, 4, 4, 24), 0, None),
    ('cspn2d_backward_history_multi_workspace_bytes', 'no history mode', (1, 2, 4, 4, 3), 0, None),
    ('cspn2d_backward_history_multi_workspace_bytes', 'no history mode (small image)', (1, 2, 17, 30, 24), 0, None),
    ('cspn2d_backward_history_multi_workspace_bytes', 'C == 1, no history mode', (1, 1, 17, 30, 24), 0, None),
    ('cspn2d_history_bytes_multi', 'too large for 32-bit indexing', (1, 3, 10000, 10000, 24), 0, None),
    ('cspn2d_multi_supported', 'bad shape', (0, 2, 64, 512, 24), 0, None),
    ('cspn2d_multi_supported', 'too large for 32-bit indexing', (1, 3, 10000, 10000, 24), 0, None),
    ('cspn2d_multi_supported', 'n_iter == 0', (2, 2, 64, 512, 0), 0, None),
    ('cspn3d_workspace_bytes', 'bad shape', (1, 0, 4, 4, 3), 0, None),
    ('cspn3d_workspace_bytes', 'n_iter == 0', (1, 2, 4, 4, 0), 0, None),
    ('cspn3d_backward_workspace_bytes', 'bad shape', (1, 0, 4, 4, 3), 0, None),
    ('cspn3d_backward_workspace_bytes', 'n_iter == 0', (1, 2, 4, 4, 0), 0, None),
    ('cspn3d_forward_absnorm_workspace_bytes', 'bad shape', (1, 0, 4, 4, 3), 0, None),
    ('cspn3d_forward_absnorm_workspace_bytes', 'n_iter == 0', (1, 2, 4, 4, 0), 0, None),
    ('cspn3d_workspace_bytes_ex', 'bad shape', (1, 2, 4, -4, 3, 2, 0), 0, None),
    ('cspn3d_workspace_bytes_ex', 'n_iter == 0', (1, 2, 4, 4, 0, 2, 0), 0, None),
    ('cspn3d_backward_multi_workspace_bytes', 'bad shape', (1, 0, 2, 4, 4, 3), 0, None),
    ('cspn3d_backward_multi_workspace_bytes', 'n_iter == 0', (1, 2, 2, 4, 4, 0), 0, None),
    ('cspn3d_multi_supported', 'bad shape', (1, 0, 2, 4, 4, 3), 0, None),
]


@pytest.fixture(scope="module")
def lib():
    _lib.load()   # (the ABI version check and the "build it first" message)
    h = ctypes.CDLL(_lib.LIB_PATH)
    h.cspn_last_error.restype = ctypes.c_char_p
    return h


def _call(lib, name, args):
    fn = getattr(lib, name)
    fn.restype = ctypes.c_size_t if name in _SIZE_T or name in _SIZE_T_EDGES else ctypes.c_int
    return fn(*[_c(a) for a in args])


@pytest.mark.parametrize("name,what,args,rc,text", ROWS, ids=["%s-%s" % (r[0], r[1].replace(" ", "_")) for r in ROWS])
def test_argument_error(lib, name, what, args, rc, text):
    # a known text first, so that the one read below is this call's
    assert _call(lib, "cspn2d_forward_f32_algo", (P(None),) * 4 + (-7, 0, 0, 0, 0, 0, P(None), Z(0), P(None))) == -1
    stale = lib.cspn_last_error()
    assert stale == b"bad shape B=-7 H=0 W=0"
    assert _call(lib, name, args) == rc
    got = lib.cspn_last_error().decode()
    if text is None:
        assert got == stale.decode()
    elif text.endswith("need "):
        assert got.startswith(text) and got[len(text)].isdigit()
    else:
        assert got == text


def test_every_3x3_entry_point_has_rows():
    names = {r[0] for r in ROWS}
    for n in ("cspn2d_forward_f32_algo", "cspn2d_backward_f32", "cspn2d_forward_history_f32", "cspn2d_backward_history_f32",
              "cspn2d_forward_multi_f32", "cspn2d_backward_multi_f32", "cspn2d_forward_history_multi_f32", "cspn2d_backward_history_multi_f32",
              "cspn3d_forward_f32_algo", "cspn3d_forward_multi_f32", "cspn3d_backward_f32", "cspn3d_backward_multi_f32",
              "cspn3d_forward_absnorm_f32"):
        assert n in names
    assert _SIZE_T <= names


def test_history_queries_where_a_history_exists(lib):
    """the shape the history rows above use: a history mode exists, one channel and two"""
    one = _call(lib, "cspn2d_history_bytes", (2, 64, 512, 24))
    assert one == 3473408 == _call(lib, "cspn2d_history_bytes_multi", (2, 1, 64, 512, 24))
    assert _call(lib, "cspn2d_history_bytes_multi", (2, 2, 64, 512, 24)) == 6881280
    assert _call(lib, "cspn2d_backward_history_workspace_bytes", (2, 64, 512, 24)) > 0
    assert _call(lib, "cspn2d_backward_history_multi_workspace_bytes", (2, 2, 64, 512, 24)) > 0


# ---- the exact edges of the size guards: the last shape each family accepts and the first it refuses ------------------------------------
# 3 x 3 in 2D: check_index32(B H W, 9); 3D: check_index32(B D H W, 27); K x K: B (K^2 - 1) H W <= 2^31 - 1
PX_2D = 0x7fffffff // 9        # 238 609 294 pixels (7.6 GB of guidance)
VX_3D = 0x7fffffff // 27       # 79 536 431 voxels (8.3 GB of gates)
PX_KXK = {5: 0x7fffffff // 24, 7: 0x7fffffff // 48}   # 89 478 485 / 44 739 242 pixels
BIG = Z(1 << 62)
_SIZE_T_EDGES = {"cspn2d_kxk_workspace_bytes", "cspn2d_kxk_history_bytes", "cspn2d_backward_kxk_workspace_bytes", "cspn2d_backward_kxk_absnorm_workspace_bytes",
            "cspn2d_kxk_norm_workspace_bytes", "cspn2d_kxk_norm_history_bytes", "cspn2d_backward_kxk_norm_workspace_bytes",
            "cspn3d_backward_g16_workspace_bytes", "cspn_guidance_head_kxk_workspace_bytes", "cspn_guidance_head_kxk_backward_workspace_bytes",
            "cspn_guidance_head_workspace_bytes", "cspn_guidance_head_backward_workspace_bytes"}
_TOO_LARGE = "tensor too large for 32-bit plane indexing"

# (symbol, arguments with the batch size left out as None, the last batch accepted at H = W (= D) = 1, the text of the refusal)
FIRST_REFUSED = [
    ("cspn2d_forward_f32_algo", (P(0x10000), P(0x20000), P(None), P(0x40000), None, 1, 1, 3, 0, 1, P(0x90000), BIG, P(None)), PX_2D, _TOO_LARGE),
    ("cspn2d_backward_f32", (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), None, 1, 1, 3, 0, P(0x90000), BIG, P(None)), PX_2D, _TOO_LARGE),
    ("cspn2d_forward_multi_f32", (P(0x10000), P(0x20000), P(None), P(0x40000), None, 2, 1, 1, 1, 3, 0, 1, P(0x90000), BIG, P(None)), PX_2D // 2, _TOO_LARGE + " (B*C*H*W)"),
    ("cspn2d_backward_multi_f32", (P(0x10000), P(0x20000), P(None), P(0x50000), P(0x60000), P(0x70000), None, 2, 1, 1, 1, 3, 0, P(0x90000), BIG, P(None)), PX_2D // 2,
     _TOO_LARGE + " (B*C*H*W)"),
    ("cspn3d_forward_f32_algo", (P(0x10000), P(0x20000), P(None), P(0x40000), None, 1, 1, 1, 3, 2, 0, P(0x90000), BIG, P(None)), VX_3D, _TOO_LARGE),
    ("cspn3d_backward_f32", (P(0x10000), P(0x20000), P(0x50000), P(0x60000), P(0x70000), None, 1, 1, 1, 3, 2, P(0x90000), BIG, P(None)), VX_3D, _TOO_LARGE),
    ("cspn3d_forward_absnorm_f32", (P(0x10000), P(0x20000), P(0x40000), None, 1, 1, 1, 3, 0, P(0x90000), BIG, P(None)), VX_3D, _TOO_LARGE),
] + [
    (name, args, PX_KXK[K], "%s: tensor too large for 32-bit element indexing" % name)
    for K in (5, 7)
    for name, args in (
        ("cspn2d_forward_kxk_f32", (P(0x10000), P(0x20000), P(0x40000), P(None), Z(0), None, 1, 1, 1, K, 3, P(0x90000), BIG, P(None))),
        ("cspn2d_backward_kxk_f32", (P(0x10000), P(0x20000), P(None), Z(0), P(0x50000), P(0x60000), P(0x70000), None, 1, 1, 1, K, 3, P(0x90000), BIG, P(None))),
        ("cspn2d_forward_kxk_absnorm_f32", (P(0x10000), P(0x20000), P(0x40000), P(None), Z(0), None, 1, 1, 1, K, 3, P(0x90000), BIG, P(None))),
        ("cspn2d_backward_kxk_absnorm_f32", (P(0x10000), P(0x20000), P(None), Z(0), P(0x50000), P(0x60000), P(0x70000), None, 1, 1, 1, K, 3, P(0x90000), BIG, P(None))),
        ("cspn2d_forward_kxk_norm_f32", (P(0x10000), P(0x20000), P(None), P(0x40000), P(None), Z(0), None, 1, 0, 1, 1, K, 3, 0, P(0x90000), BIG, P(None))),
        ("cspn2d_backward_kxk_norm_f32", (P(0x10000), P(0x20000), P(None), P(None), Z(0), P(0x50000), P(0x60000), P(0x70000), None, 1, 0, 1, 1, K, 3, 0, P(0x90000), BIG,
                                          P(None))),
    )
]


@pytest.mark.parametrize("name,args,last,text", FIRST_REFUSED, ids=["%s-%d" % (r[0], r[2]) for r in FIRST_REFUSED])
def test_first_refused_shape(lib, name, args, last, text):
    """one element over the limit: refused with CSPN_E_UNSUPPORTED before anything is launched (the pointers are fake).  The last accepted
    shape is asked of the size queries below, which launch nothing"""
    assert _call(lib, name, tuple(last + 1 if a is None else a for a in args)) == -3
    assert lib.cspn_last_error().decode() == text


def test_size_queries_at_the_last_accepted_shape_2d(lib):
    """the sizes in 64-bit Python integers: no query returns 0 or a wrapped value for the last shape the entry points accept"""
    for shape in ((PX_2D, 1, 1), (1, 2, PX_2D // 2), (366, 304, 1216)):
        px = shape[0] * shape[1] * shape[2]
        for n_iter in (1, 3, 24, 48):
            # the per-step forward: 9 folded planes + two value planes; the query covers every algo (>= that)
            assert _call(lib, "cspn2d_workspace_bytes", shape + (n_iter,)) >= 11 * 4 * px
            # past the line the backward takes its per-step path: 9 + 8 folded planes, n_iter - 1 levels, n_iter adjoint levels
            assert _call(lib, "cspn2d_backward_workspace_bytes", shape + (n_iter,)) == (9 + 8 + 2 * n_iter - 1) * 4 * px
            assert _call(lib, "cspn2d_history_bytes", shape + (n_iter,)) == 0
            assert _call(lib, "cspn2d_backward_history_workspace_bytes", shape + (n_iter,)) == 0
    # the largest batch of 304 x 1216 images whose 8 folded planes stay below 2^32 bytes keeps the ring path and its history; one more does not
    assert 363 * 304 * 1216 * 32 < 1 << 32 <= 364 * 304 * 1216 * 32
    assert _call(lib, "cspn2d_history_bytes", (363, 304, 1216, 24)) == 65536 + 13 * 4 * 363 * 304 * 1216
    assert _call(lib, "cspn2d_history_bytes", (364, 304, 1216, 24)) == 0
    # C channels on shared guidance: the limit is on B C H W
    assert _call(lib, "cspn2d_workspace_bytes_multi", (PX_2D // 2, 2, 1, 1, 3)) >= 11 * 4 * (PX_2D // 2)
    assert _call(lib, "cspn2d_backward_multi_workspace_bytes", (PX_2D // 2, 2, 1, 1, 3)) >= (9 + 8 + 5) * 4 * (PX_2D // 2)
    assert _call(lib, "cspn2d_multi_supported", (PX_2D // 2 + 1, 2, 1, 1, 3)) == 0


def test_size_queries_at_the_last_accepted_shape_3d(lib):
    small = _call(lib, "cspn3d_workspace_bytes", (1, 2, 4, 4, 3)) - 29 * 4 * 32   # the exchange buffers and sync words: a constant
    assert 0 < small < 1 << 26
    for shape in ((VX_3D, 1, 1, 1), (16, 32, 160, 608)):
        vx = shape[0] * shape[1] * shape[2] * shape[3]
        # 27 folded planes + two value volumes + that constant
        assert _call(lib, "cspn3d_workspace_bytes", shape + (3,)) == 29 * 4 * vx + small
        assert _call(lib, "cspn3d_workspace_bytes_ex", shape + (3, 0, 0)) == 29 * 4 * vx + small
        # the Paddle contract on W % 4 == 0 folds nothing
        assert _call(lib, "cspn3d_workspace_bytes_ex", shape + (3, 2, 0)) == (2 if shape[3] % 4 == 0 else 29) * 4 * vx + small
        assert _call(lib, "cspn3d_forward_absnorm_workspace_bytes", shape + (3,)) >= (26 + 2) * 4 * vx
        for q in ("cspn3d_backward_workspace_bytes", "cspn3d_backward_g16_workspace_bytes"):
            assert _call(lib, q, shape + (2,)) >= 3 * 4 * vx   # one kept level and two value volumes at the least
    # the persistent kernel indexes the gates with 32-bit byte offsets: it declines every batch of 4 GiB of gates or more (without a device
    # its residency test may decline too: tests/test_past_4gib.py holds the batch just below the line against the one just past it on the GPU)
    assert _call(lib, "cspn3d_multi_supported", (16, 1, 32, 160, 608, 12)) == 0


@pytest.mark.parametrize("K", [5, 7])
def test_size_queries_at_the_last_accepted_shape_kxk(lib, K):
    px = PX_KXK[K]
    for shape in ((1, 1, 1, px), (px, 1, 1, 1)):
        assert _call(lib, "cspn2d_kxk_history_bytes", shape + (K, 3)) == 2 * 4 * px == _call(lib, "cspn2d_kxk_norm_history_bytes", shape + (K, 3))
        assert 2 * 4 * px <= _call(lib, "cspn2d_kxk_workspace_bytes", shape + (K, 3)) < 2 * 4 * px + 4096
        assert 2 * 4 * px <= _call(lib, "cspn2d_backward_kxk_workspace_bytes", shape + (K, 3)) < 2 * 4 * px + 256
        assert _call(lib, "cspn2d_backward_kxk_absnorm_workspace_bytes", shape + (K, 3)) >= 3 * 4 * px
        # folded planes: K^2 - 1 weights + the bias (+ the levels)
        assert _call(lib, "cspn2d_kxk_norm_workspace_bytes", shape[:2] + (0,) + shape[2:] + (K, 3)) >= (K * K + 2) * 4 * px
        assert _call(lib, "cspn2d_backward_kxk_norm_workspace_bytes", shape[:2] + (0,) + shape[2:] + (K, 3)) >= (2 * K * K + 2) * 4 * px
        over = (shape[0], 1, 1, shape[3] + 1) if shape[0] == 1 else (shape[0] + 1, 1, 1, 1)
        for q in ("cspn2d_kxk_history_bytes", "cspn2d_kxk_workspace_bytes", "cspn2d_backward_kxk_workspace_bytes", "cspn2d_backward_kxk_absnorm_workspace_bytes"):
            assert _call(lib, q, over + (K, 3)) == 0


@pytest.mark.parametrize("K,B_last", [(5, (1 << 40) // (24 << 24)), (7, (1 << 40) // (48 << 24))])
def test_first_refused_shape_of_the_kxk_heads(lib, K, B_last):
    """the heads index with size_t and refuse at B (K^2 - 1) H W >= 2^40: 4096 x 4096 outputs, the first batch over the limit, forward and backward"""
    assert B_last * (K * K - 1) << 24 < 1 << 40 <= (B_last + 1) * (K * K - 1) << 24
    fwd = (P(0x10000), P(0x20000), P(None), P(0x40000), P(None), B_last + 1, 1, 2048, 2048, 4096, 4096, K, P(0x90000), BIG, P(None))
    assert _call(lib, "cspn_guidance_head_kxk_f32", fwd) == -3
    assert lib.cspn_last_error().decode() == "cspn_guidance_head_kxk_f32: tensor too large"
    bwd = (P(0x10000), P(0x20000), P(None), P(0x50000), P(None), P(0x60000), P(None), P(None), B_last + 1, 1, 2048, 2048, 4096, 4096, K, P(0x90000), BIG, P(None))
    assert _call(lib, "cspn_guidance_head_kxk_backward_f32", bwd) == -3
    assert lib.cspn_last_error().decode() == "cspn_guidance_head_kxk_backward_f32: tensor too large"
    assert _call(lib, "cspn_guidance_head_kxk_workspace_bytes", (B_last, 1, 2048, 2048, K)) > 0
    assert _call(lib, "cspn_guidance_head_kxk_backward_workspace_bytes", (B_last, 1, 2048, 2048, K)) > 0


def test_first_refused_shape_of_the_3x3_heads(lib):
    """cspn_guidance_head_f32 and its backward index with size_t and refuse at B 8 H W >= 2^40: 4096 x 4096 outputs, B = 2^13 is the first batch
    over the limit (refused behind the argument and workspace checks, before any launch; the batch before it would launch, so it is asked of the
    size queries only)"""
    B_last, C = (1 << 40) // (8 << 24) - 1, 1
    assert B_last == (1 << 13) - 1 and B_last * 8 << 24 < 1 << 40 <= (B_last + 1) * 8 << 24
    fwd = (P(0x10000), P(0x20000), P(None), P(0x40000), P(None), B_last + 1, C, 2048, 2048, 4096, 4096, 2, P(0x90000), BIG, P(None))
    assert _call(lib, "cspn_guidance_head_f32", fwd) == -3
    assert lib.cspn_last_error().decode() == "tensor too large"
    bwd = (P(0x10000), P(0x20000), P(None), P(0x50000), P(None), P(0x60000), P(None), P(None), B_last + 1, C, 2048, 2048, 4096, 4096, P(0x90000), BIG, P(None))
    assert _call(lib, "cspn_guidance_head_backward_f32", bwd) == -3
    assert lib.cspn_last_error().decode() == "tensor too large"
    # one element under the limit in the other direction too: the same batch at 4096 x 4095 passes the size test and stops at the workspace
    small = (P(0x10000), P(0x20000), P(None), P(0x50000), P(None), P(0x60000), P(None), P(None), B_last + 1, C, 2048, 2048, 4096, 4095, P(0x90000), Z(0), P(None))
    assert _call(lib, "cspn_guidance_head_backward_f32", small) == -2
    assert lib.cspn_last_error().decode().startswith("workspace: need ")
    assert 0 < _call(lib, "cspn_guidance_head_workspace_bytes", (C,)) < 1 << 40
    for B in (B_last, B_last + 1):
        assert 0 < _call(lib, "cspn_guidance_head_backward_workspace_bytes", (B, C, 2048, 2048)) < 1 << 50


def test_channels_on_shared_guidance_cannot_reach_the_line(lib):
    """C >= 2 channels on shared guidance: the limit is on B C H W (check_index32), so the guidance of the largest batch accepted stays below
    4 GiB and its descriptors' high dword stays 0 -- nothing to run past the line"""
    assert 32 * (PX_2D // 2) < 1 << 32
    B = (1 << 32) // 32 // (304 * 1216) + 1     # the first batch of KITTI images with 4 GiB of guidance
    assert 32 * B * 304 * 1216 >= 1 << 32 and 2 * B * 304 * 1216 > PX_2D
    assert _call(lib, "cspn2d_multi_supported", (B, 2, 304, 1216, 24)) == 0
    args = (P(0x10000), P(0x20000), P(None), P(0x40000), B, 2, 1, 304, 1216, 24, 0, 0, P(0x90000), BIG, P(None))
    assert _call(lib, "cspn2d_forward_multi_f32", args) == -3
    assert lib.cspn_last_error().decode() == _TOO_LARGE + " (B*C*H*W)"
