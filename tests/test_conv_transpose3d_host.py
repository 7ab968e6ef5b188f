"""Host-side checks of CplxConvTranspose3d and the C ABI of csrc/conv3d.hip (no GPU): the layer's surface against the
reference's recorded state dict, the library's geometry answers, and the facts the exactness argument of
test_gpu_conv_transpose3d.py rests on."""
import ctypes

import numpy as np
import pytest
import torch

import conv_transpose3d_cases as K
from conv_transpose3d_cases import CASES

EINVAL, ESHAPE = -1, -3


def _geom(*v):
    assert len(v) == 19
    return (ctypes.c_int * 19)(*v)


def _lib():
    from cplxmodule_amd import _lib
    return _lib.load()


def _out_shape(geom):
    out = (ctypes.c_int * 3)()
    rc = _lib().cplxamd_conv3d_out_shape(geom, ctypes.byref(out, 0), ctypes.byref(out, 4), ctypes.byref(out, 8))
    return rc, tuple(out)


# ---- the layer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,kw", [("nobias", {}), ("bias", {"bias": True})])
def test_layer_state_dict_matches_the_reference(golden, tag, kw):
    from cplxmodule_amd.nn import CplxConvTranspose3d
    from cplxmodule_amd.nn.modules import CplxConvTranspose3d as same
    assert same is CplxConvTranspose3d
    g = golden("conv_transpose3d")
    layer = CplxConvTranspose3d(4, 6, 3, stride=2, padding=1, **kw)
    sd = layer.state_dict()
    assert sorted(sd) == sorted(str(k) for k in g[f"layer_{tag}_keys"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(int(n) for n in g[f"layer_{tag}_shape_{k}"]), k
    assert (layer.bias is None) == (tag == "nobias")             # the reference's default: bias=None
    assert layer.kernel_size == (3, 3, 3) and layer.stride == (2, 2, 2) and layer.output_padding == (0, 0, 0)
    assert layer.transposed and tuple(layer.weight.shape) == (4, 6, 3, 3, 3)
    r = layer.extra_repr()
    assert "kernel_size=(3, 3, 3)" in r and "stride=(2, 2, 2)" in r and ("bias=False" in r) == (tag == "nobias")
    assert "CplxConvTranspose3d" in repr(layer)


def test_layer_constructor_is_the_references():
    from cplxmodule_amd.nn import CplxConvTranspose1d, CplxConvTranspose2d, CplxConvTranspose3d
    layer = CplxConvTranspose3d(4, 6, (2, 3, 4), (1, 2, 3), (0, 1, 2), (2, 1, 1), (0, 1, 2), 2, True, "circular")
    assert layer.kernel_size == (2, 3, 4) and layer.stride == (1, 2, 3) and layer.padding == (0, 1, 2)
    assert layer.dilation == (2, 1, 1) and layer.output_padding == (0, 1, 2) and layer.groups == 2
    assert layer.padding_mode == "circular" and tuple(layer.weight.shape) == (4, 3, 2, 3, 4) and tuple(layer.bias.shape) == (6,)
    assert "output_padding=(0, 1, 2)" in layer.extra_repr()
    with pytest.raises(ValueError):
        CplxConvTranspose3d(4, 6, 3, groups=3)
    with pytest.raises(ValueError):
        CplxConvTranspose3d(4, 6, 3, padding_mode="reflect")
    # the 1-d and 2-d layers behave as before
    assert CplxConvTranspose2d(4, 6, 3).kernel_size == (3, 3) and CplxConvTranspose1d(4, 6, 3).kernel_size == (3,)
    assert tuple(CplxConvTranspose2d(4, 6, 3, groups=2).weight.shape) == (4, 3, 3, 3)


def test_output_size_resolution():
    from cplxmodule_amd.nn import CplxConvTranspose3d
    layer = CplxConvTranspose3d(4, 6, 3, stride=2, padding=1)
    x = torch.empty(2, 4, 3, 4, 5)
    assert layer._resolve_output_padding(x, None) == (0, 0, 0)
    # valid sizes of dim n: lo = (L - 1) 2 - 2 + 2 + 1 = 2 L - 1 and lo + 1
    for size, pads in (((5, 7, 9), (0, 0, 0)), ((6, 8, 10), (1, 1, 1)), ((5, 8, 9), (0, 1, 0)), ((6, 7, 10), (1, 0, 1)),
                       ((2, 6, 6, 8, 9), (1, 1, 0))):
        assert layer._resolve_output_padding(x, size) == pads, size
    for size in ((7, 8, 10), (6, 8, 11), (4, 7, 9)):
        with pytest.raises(ValueError):
            layer._resolve_output_padding(x, size)
    # dilation above the stride widens the range
    wide = CplxConvTranspose3d(4, 6, 2, stride=1, dilation=3)
    assert wide._resolve_output_padding(x, (8, 9, 10)) == (2, 2, 2)
    with pytest.raises(ValueError):
        wide._resolve_output_padding(x, (9, 9, 10))


def test_cpu_tensors_raise():
    from cplxmodule_amd import Cplx, cplx
    from cplxmodule_amd._lib import CplxAmdError
    from cplxmodule_amd.nn import CplxConvTranspose3d
    x = Cplx(torch.randn(1, 4, 2, 3, 4), torch.randn(1, 4, 2, 3, 4))
    with pytest.raises(CplxAmdError):
        CplxConvTranspose3d(4, 6, 3)(x)
    w = Cplx(torch.randn(4, 3, 2, 2, 2), torch.randn(4, 3, 2, 2, 2))
    for mode in ("zeros", "circular"):
        with pytest.raises(CplxAmdError):
            cplx.conv_transpose3d(x, w, None, padding=1, groups=2, padding_mode=mode)


def test_functional_argument_checks():
    from cplxmodule_amd import Cplx, cplx
    x = Cplx(torch.randn(1, 4, 2, 3, 4), torch.randn(1, 4, 2, 3, 4))
    w = Cplx(torch.randn(4, 3, 2, 2, 2), torch.randn(4, 3, 2, 2, 2))
    with pytest.raises(ValueError, match="output_padding"):
        cplx.conv_transpose3d(x, w, None, stride=2, output_padding=2)
    with pytest.raises(ValueError, match="output_padding"):
        cplx.conv_transpose3d(x, w, None, stride=(1, 2, 2), output_padding=(1, 0, 0))
    with pytest.raises(ValueError, match="padding_mode"):
        cplx.conv_transpose3d(x, w, None, padding_mode="reflect")
    import inspect
    sig = inspect.signature(cplx.conv_transpose3d)
    assert list(sig.parameters) == ["input", "weight", "bias", "stride", "padding", "output_padding", "groups", "dilation",
                                    "padding_mode"]
    assert sig.parameters["groups"].default == 1                 # (not the reference's 0)


def test_conv_transposend_names_the_dimensionality():
    import torch.nn.functional as F
    from cplxmodule_amd import Cplx, cplx
    from cplxmodule_amd._lib import CplxAmdError
    x3 = Cplx(torch.randn(1, 4, 2, 3, 4), torch.randn(1, 4, 2, 3, 4))
    w3 = Cplx(torch.randn(4, 3, 2, 2, 2), torch.randn(4, 3, 2, 2, 2))
    x2 = Cplx(torch.randn(1, 4, 3, 4), torch.randn(1, 4, 3, 4))
    w2 = Cplx(torch.randn(4, 3, 2, 2), torch.randn(4, 3, 2, 2))
    for fn in (F.conv_transpose2d, F.conv_transpose1d, cplx.conv_transpose2d):
        with pytest.raises(ValueError):
            cplx.conv_transposend(fn, x3, w3)
        with pytest.raises(ValueError):
            cplx.conv_transposend_naive(fn, x3, w3)
        with pytest.raises(ValueError):
            cplx.conv_transposend_3m(fn, x3, w3)
    with pytest.raises(ValueError):
        cplx.conv_transposend(F.conv_transpose3d, x2, w2)
    # the right name (or None) reaches the package's own function, which has no CPU path
    for fn in (F.conv_transpose3d, cplx.conv_transpose3d, None):
        with pytest.raises(CplxAmdError):
            cplx.conv_transposend(fn, x3, w3)
    with pytest.raises(CplxAmdError):
        cplx.conv_transposend_naive(F.conv_transpose2d, x2, w2)
    with pytest.raises(CplxAmdError):
        cplx.conv_transposend_3m(None, x3, w3, 1, 0, 0, 1, 1)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def _torch_out(L, k, s, p, d):
    return (L + 2 * p - d * (k - 1) - 1) // s + 1


def test_out_shape_agrees_with_torch_formula():
    table = []
    for c in CASES.values():                                     # the correlation of a case maps the layer's output back
        table.append((K.out_dhw(c), c["k"], c["stride"], K.eff_padding(c), c["dilation"], K.in_dhw(c)))
    for dhw, k, s, p, d in K.EXTRA_GEOMETRIES:
        table.append((dhw, k, s, p, d, None))
    for dhw, k, s, p, d, want in table:
        rc, got = _out_shape(_geom(2, 4, 6, *dhw, *k, *s, *p, *d, 2))
        assert rc == 0, (dhw, k, s, p, d)
        assert got == tuple(_torch_out(L, kk, ss, pp, dd) for L, kk, ss, pp, dd in zip(dhw, k, s, p, d))
        if want is not None:
            assert got == tuple(want)
        ref = torch.nn.functional.conv3d(torch.zeros(1, 1, *dhw), torch.zeros(1, 1, *k), None, s, p, d)
        assert got == tuple(ref.shape[2:])


BAD_GEOMETRIES = {
    "groups do not divide Ci": (2, 5, 6, 4, 4, 4, 3, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2),
    "groups do not divide Co": (2, 4, 7, 4, 4, 4, 3, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2),
    "zero stride": (2, 4, 6, 4, 4, 4, 3, 3, 3, 1, 0, 1, 0, 0, 0, 1, 1, 1, 2),
    "zero dilation": (2, 4, 6, 4, 4, 4, 3, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 0, 2),
    "zero groups": (2, 4, 6, 4, 4, 4, 3, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 1, 0),
    "empty output": (2, 4, 6, 2, 4, 4, 3, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2),
    "empty output, stride 2 (numerator -1)": (2, 4, 6, 4, 4, 1, 3, 3, 2, 2, 2, 2, 0, 0, 0, 1, 1, 1, 2),
    "negative batch": (-1, 4, 6, 4, 4, 4, 3, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2),
    "B D H W beyond 32 bits": (64, 4, 6, 512, 512, 512, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2),
    "D H W beyond 32 bits": (1, 4, 6, 2048, 2048, 2048, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2),
    "taps beyond 32 bits": (1, 4, 6, 2048, 2048, 2048, 2048, 2048, 2048, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2),
}


@pytest.mark.parametrize("what", list(BAD_GEOMETRIES))
def test_invalid_geometry_is_rejected_not_crashed(what):
    L = _lib()
    geom = _geom(*BAD_GEOMETRIES[what])
    rc, _ = _out_shape(geom)
    assert rc in (EINVAL, ESHAPE), what
    assert L.cplxamd_conv3d_wgrad_ws_bytes(geom) == -1
    # the launchers check the geometry before they touch a pointer or the device
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (0, 1):
        assert L.cplxamd_conv3d_fwd(p, p, p, p, p, p, geom, dt, None) in (EINVAL, ESHAPE)
        assert L.cplxamd_conv3d_dgrad(p, p, p, p, None, None, p, p, geom, dt, 0, None) in (EINVAL, ESHAPE)
        assert L.cplxamd_conv3d_wgrad(p, p, p, p, p, p, geom, dt, p, 64, None) in (EINVAL, ESHAPE)


def test_null_pointers_and_bad_codes_are_rejected_not_crashed():
    L = _lib()
    geom = _geom(2, 4, 6, 4, 4, 4, 3, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    out = (ctypes.c_int * 3)()
    assert L.cplxamd_conv3d_out_shape(None, out, out, out) == EINVAL
    assert L.cplxamd_conv3d_out_shape(geom, None, out, out) == EINVAL
    assert L.cplxamd_conv3d_wgrad_ws_bytes(None) == -1
    for hole in range(6):                                        # each plane in turn, the imaginary ones included: complex only
        a = [p] * 6
        a[hole] = None
        assert L.cplxamd_conv3d_fwd(*a, geom, 0, None) == EINVAL, hole
        assert L.cplxamd_conv3d_dgrad(*a[:4], None, None, *a[4:], geom, 0, 0, None) == EINVAL, hole
        assert L.cplxamd_conv3d_wgrad(*a, geom, 0, p, 1 << 20, None) == EINVAL, hole
    assert L.cplxamd_conv3d_fwd(p, p, p, p, p, p, None, 0, None) == EINVAL
    assert L.cplxamd_conv3d_wgrad(p, p, p, p, p, p, geom, 0, None, 0, None) == EINVAL          # no workspace
    assert L.cplxamd_conv3d_dgrad(p, p, p, p, p, None, p, p, geom, 0, 0, None) == EINVAL       # half a bias
    assert L.cplxamd_conv3d_dgrad(p, p, p, p, None, None, p, p, geom, 0, 2, None) == EINVAL    # unknown flag
    for bad_dtype in (2, 3, -1):                                 # IEEE half, float64: no such form
        assert L.cplxamd_conv3d_fwd(p, p, p, p, p, p, geom, bad_dtype, None) == EINVAL
        assert L.cplxamd_conv3d_dgrad(p, p, p, p, None, None, p, p, geom, bad_dtype, 0, None) == EINVAL
        assert L.cplxamd_conv3d_wgrad(p, p, p, p, p, p, geom, bad_dtype, p, 1 << 20, None) == EINVAL
    # an empty batch returns before any launch
    empty = _geom(0, 4, 6, 4, 4, 4, 3, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 1, 2)
    assert L.cplxamd_conv3d_fwd(p, p, p, p, p, p, empty, 0, None) == 0
    assert L.cplxamd_conv3d_dgrad(p, p, p, p, None, None, p, p, empty, 1, 0, None) == 0


def test_split_k_case_uses_several_slabs():
    c = CASES["splitk"]
    geom = _geom(*K.geom_of(c))
    wsz = int(np.prod(K.shapes(c)[1]))
    nbytes = _lib().cplxamd_conv3d_wgrad_ws_bytes(geom)
    slabs = nbytes // (2 * 4 * wsz)                              # [2 planes][splits] float32 slabs of the weight's size
    assert slabs > 1, (nbytes, wsz)
    for c in CASES.values():                                     # and every case's query answers
        assert _lib().cplxamd_conv3d_wgrad_ws_bytes(_geom(*K.geom_of(c))) >= 2 * 4 * int(np.prod(K.shapes(c)[1]))


# ---- the exactness argument rests on checked facts ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_is_exactly_representable(name):
    c = CASES[name]
    d, ref = K.reference(c)
    xs, ws, ys = K.shapes(c)
    assert ref["yr"].shape == ys and ref["dxr"].shape == xs and ref["dwr"].shape == ws
    # the reference was computed for the geometry the library will be handed: its correlation maps y's extent back to x's
    assert _out_shape(_geom(*K.geom_of(c))) == (0, K.in_dhw(c))
    for k, v in ref.items():
        assert np.array_equal(v * 2, np.round(v * 2)), f"{k}: not integers or half-integers"
        assert np.abs(v).max() < 2 ** 24, k
        K.expected(v, "f32")                                     # (asserts the float32 round trip)
    for k, v in d.items():
        lim = {"x": 3, "w": 2, "g": 3, "b": 8}[k[0]]
        assert np.abs(v).max() <= lim and np.array_equal(v * 2, np.round(v * 2)), k
    tf, td, tw = K.terms(c)
    for Kdim in (tf, td):
        assert 2 * Kdim * 6 + 8 < 2 ** 24
    assert K.magnitude_bound(c) < 2 ** 24
    # the sums are not trivially zero: most outputs are non-zero, so a dropped tap shows
    assert (ref["yr"] != 0).mean() > 0.25 or name.startswith("empty_phase")


def test_circular_case_has_the_recorded_shape(golden):
    g = golden("conv_transpose3d")
    assert g["circular_yr"].shape == (2, 6, 7, 8, 9)
    c = CASES["circular"]
    assert K.in_dhw(c) == (6, 6, 6) and K.out_dhw(c) == (7, 8, 9)
    from cplxmodule_amd.conv3d import _circular_pads
    assert _circular_pads(c["padding"]) == K.pads_of(c) == (1, 0, 1, 1, 2, 1)      # W first: padding[0] wraps W
