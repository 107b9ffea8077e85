"""Weight-panel geometries with the pack kernel each one must reach (TEST INFRASTRUCTURE; never imported by the package, no GPU
import).

A convolution entry point re-lays its weights out into a panel before it launches.  Four sites do that, and the job that
``zsv_conv3d_panel_job`` writes down names the site by its ``kind``: 0 the direct kernel's panel (conv_tap.hip), 1 a Winograd
F(2,3) panel, 2 a Winograd F(4,3) panel (both Winograd sites of conv_wino.hip: along W and along T), 3 the panel of the strided
input gradient (conv_dgrad_s2.hip).  Which site a geometry reaches depends on tile-count thresholds, so a small geometry with a
Winograd name can still take the direct kernel: every row here carries the kinds it must record for (forward, forward with a
bias / ReLU / statistics, input gradient), and the switches that lower the thresholds far enough for its size.

``tests/test_panel_host.py`` checks the kinds, sizes and refusals without a GPU (query and job launch nothing and dereference
nothing); ``tests/test_ops_gpu.py::test_weight_panels_packed_ahead_of_the_call`` runs the kernels on the same rows.
"""
from collections import namedtuple

PanelCase = namedtuple("PanelCase", "name xs ws stride padding switches kinds")

VARIANTS = [(0, 0), (0, 1), (1, 0)]           # (direction, extras) of the three kinds of a row, in order

_F43 = ((3, 64, 4, 24, 24), (144, 64, 1, 3, 3), 1, (0, 1, 1))
_VW7 = ((6, 96, 2, 7, 7), (200, 96, 1, 3, 3), 1, (0, 1, 1))
_WINOT = ((3, 144, 8, 16, 16), (64, 144, 3, 1, 1), 1, (1, 0, 0))
_FULL = ((2, 32, 6, 12, 16), (48, 32, 3, 3, 3), 1, (1, 1, 1))
_T1 = ((2, 144, 8, 32, 32), (64, 144, 3, 1, 1), 1, (1, 0, 0))     # 2.4 M input elements: the largest row

# rows that reach the Winograd sites (and the direct kernel's site through the BatchNorm-folded forward): geometries of
# test_ops_gpu.PANEL_CASES, which at default switches all lie below the Winograd kernels' tile thresholds
SWITCHED_CASES = [
    PanelCase("winograd_f43-f43", *_F43, {"ZSV_WINO_MIN_TILES": "1"}, (2, 2, 2)),
    PanelCase("winograd_f43-f23", *_F43, {"ZSV_WINO_MIN_TILES": "1", "ZSV_WINO_NO_F43": "1"}, (1, 1, 1)),
    PanelCase("virtual_width_7-f43", *_VW7, {"ZSV_WINO_VW_MIN_WGS": "1"}, (2, 2, 2)),
    PanelCase("temporal_winograd-f43", *_WINOT, {"ZSV_WINOT_MIN_TILES": "1"}, (2, 2, 2)),
    PanelCase("temporal_winograd-f23", *_WINOT, {"ZSV_WINOT_MIN_TILES": "1", "ZSV_WINOT_NO_F43": "1"}, (1, 1, 1)),
    PanelCase("full_333-f43", *_FULL, {"ZSV_WINO_MIN_TILES": "1"}, (2, 2, 2)),
    PanelCase("bn_folded_t1_like", *_T1, {}, (0, 0, 0)),
    PanelCase("bn_folded_t1_like-f43", *_T1, {"ZSV_WINOT_MIN_TILES": "1"}, (2, 2, 2)),
]
PRE_SUPPORTED = {"bn_folded_t1_like", "bn_folded_t1_like-f43"}    # zsv_conv3d_pre_supported is 1 for these


def default_kinds(name):
    """Kinds of a row of test_ops_gpu.PANEL_CASES at default switches: the direct kernel, but for the two strided dgrads."""
    return (0, 0, 3) if name in ("strided_spatial", "strided_temporal") else (0, 0, 0)


def rows(panel_cases):
    """test_ops_gpu.PANEL_CASES at default switches, then SWITCHED_CASES."""
    return [PanelCase(*c, {}, default_kinds(c[0])) for c in panel_cases] + SWITCHED_CASES


# no single panel: query answers 0 bytes with ZSV_OK, job and the *_panel forms refuse with ZSV_E_UNSUPPORTED
STEM = ((2, 3, 4, 32, 32), (45, 3, 1, 7, 7), (1, 2, 2), (0, 3, 3))                 # generic kernel, forward and input gradient
NO_PANEL = [
    # name, x shape, w shape, stride, padding, direction
    ("stem_forward", *STEM, 0),
    ("stem_dgrad", *STEM, 1),
    ("pointwise_stride2_dgrad", (3, 64, 4, 12, 12), (128, 64, 1, 1, 1), (2, 2, 2), (0, 0, 0), 1),      # class by class
    ("full_333_stride2_dgrad", (2, 32, 6, 12, 16), (48, 32, 3, 3, 3), (2, 2, 2), (1, 1, 1), 1),        # class by class
]
