"""cspn_amd -- MI355X-native CSPN propagation engine (hand-written HIP for gfx950).

Scope: the one hot path of XinJCheng/CSPN -- Affinity_Propagate
(reference cspn_pytorch/models/cspn.py:14-83) and its 3D call site
(reference cspn_paddle/demo.py:41-52).  See DESIGN.md / INTEGRATION.md."""
from ._lib import CspnError, build, load  # noqa: F401
from .cspn import CSPN, Affinity_Propagate, Affinity_Propagate3d, Affinity_PropagateAssemble, Affinity_PropagateKxK, propagate_prenorm  # noqa: F401
from .functional import (affinity_propagate, cspn2d_backward, cspn2d_forward_sited8, guidance_to_sited8, cspn2d_normalize, cspn2d_normalize_backward, cspn2d_backward_from_history, cspn2d_forward,  # noqa: F401
                         cspn2d_forward_with_history, cspn2d_history_bytes, cspn2d_forward_multi, cspn2d_backward_multi, cspn2d_multi_supported, cspn3d_forward, cspn3d_forward_multi, cspn3d_backward, cspn3d_backward_multi, cspn3d_backward_norm, cspn3d_forward_norm, cspn3d_check_status,
                         gate_absnorm, absnorm_propagate, cspn2d_forward_kxk, cspn2d_backward_kxk, cspn2d_forward_kxk_norm,
                         cspn2d_backward_kxk_norm, cspn2d_forward_kxk_absnorm, cspn2d_backward_kxk_absnorm, cspn2d_forward_kxk_assemble,
                         cspn2d_backward_kxk_assemble)
from .train_utils import GuidanceHeads, guidance_heads, guidance_heads_backward  # noqa: F401
# non-local propagation: importable from the package, its functions are cspn_amd.functional.cspn2d_*_nl* (not in __all__: DESIGN.md §3.4j)
from .nlspn import NonLocal_Propagate  # noqa: F401
# K x K propagation with per-step attention: importable from the package, its functions are cspn_amd.functional.cspn2d_*_kxk_dyn (not in
# __all__: DESIGN.md §3.4k)
from .dyspn import Dynamic_Propagate  # noqa: F401
# line-scan propagation (SPN's three-way recurrence): importable from the package, its functions are cspn_amd.functional.cspn2d_*_scan (not in
# __all__: DESIGN.md §3.4l)
from .spn import LineScan_Propagate  # noqa: F401

__all__ = ["Affinity_Propagate", "Affinity_Propagate3d", "Affinity_PropagateKxK", "propagate_prenorm", "cspn2d_forward", "cspn2d_normalize", "cspn2d_normalize_backward", "cspn2d_backward", "cspn2d_forward_multi", "cspn2d_backward_multi", "cspn3d_forward", "cspn3d_forward_multi", "cspn3d_backward", "cspn3d_backward_multi", "cspn3d_backward_norm", "cspn3d_forward_norm", "cspn3d_check_status", "affinity_propagate",
           "CSPN", "gate_absnorm", "absnorm_propagate", "cspn2d_forward_kxk", "cspn2d_backward_kxk", "cspn2d_forward_kxk_norm",
           "cspn2d_backward_kxk_norm", "cspn2d_forward_kxk_absnorm", "cspn2d_backward_kxk_absnorm", "cspn2d_forward_kxk_assemble",
           "cspn2d_backward_kxk_assemble", "Affinity_PropagateAssemble", "guidance_heads", "guidance_heads_backward", "GuidanceHeads", "build", "load",
           "CspnError"]
