"""grid= / origin= / roi= on tt.simulate(.., binary=False), tt.intensity and tt.loss: a real leaf of any
size zero-filled into one of the built grids, the outputs and the loss taken over a rectangle of it.

Checked against the float64 oracle on the explicitly embedded array, sliced: the forward within the
project's bounds (field and intensity 2e-5 of the maximum, MSE 2.31e-5 relative, PSNR 1e-4 dB), and
x.grad within 2e-5 of max|want| with
    want = crop_in Re A(-z)[embed_out((2 / P) gI F)]     (times vb s(x) for a thresholded leaf),
the formulation that agreed with central differences in float64 (tests/test_window_host.py restates
the check).  Also: the result equals the full-grid route (F.pad, the unwindowed call, a slice) bit for
bit, and sixteen Adam steps through tt.loss(.., threshold=0.5, grid=64, roi=..) lower the loss."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, loss_coeffs  # noqa: E402
from tests.test_threshold_ste_host import STE_WINDOW, binarize, field_values, ste_surrogate  # noqa: E402

Z = 2e-3
WL = 515e-9
TAU = 0.5
FIELD_RTOL = 2e-5
PSNR_ATOL = 1e-4
MSE_RTOL = 2.31e-5
FIELD = {"amplitude": O.FIELD_AMPLITUDE, "phase": O.FIELD_PHASE}
UP = np.array([1.0, -0.5])

# name: (grid, leaf shape [B, C, h, w], wavelengths, origin | None, roi | None)
CASES = {
    "mono": (64, (2, 2, 40, 33), (WL,), (5, 9), (3, 20, 50, 31)),
    "rgb": (64, (1, 6, 40, 33), tuple(O.WL_RGB), (5, 9), (3, 20, 50, 31)),
    "centred256": (256, (1, 2, 150, 201), (WL,), None, None),       # a rectangular hologram, all defaults
}


def _meta(wls):
    return {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wls[0] if len(wls) == 1 else tuple(wls)}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _windows(name):
    n, shape, _, origin, roi = CASES[name]
    h, w = shape[2:]
    y0, x0 = origin if origin is not None else ((n - h) // 2, (n - w) // 2)
    in_win = (y0, x0, h, w)
    return in_win, (roi if roi is not None else in_win)


def _kw(name):
    n, _, _, origin, roi = CASES[name]
    return {"grid": n, "origin": origin, "roi": roi}


def embed(a, win, n):
    y0, x0, h, w = win
    out = np.zeros(a.shape[:-2] + (n, n), a.dtype)
    out[..., y0:y0 + h, x0:x0 + w] = a
    return out


def crop(a, win):
    y0, x0, h, w = win
    return a[..., y0:y0 + h, x0:x0 + w]


@functools.lru_cache(maxsize=None)
def _case(name):
    """x float32 leaf in [-0.5, 1.5] with tau and the default gate's ends planted; target f32 over the roi;
    a complex upstream w and a real one gi over the roi; the G transfer functions of the grid.  Read-only."""
    n, shape, wls, _, _ = CASES[name]
    b, c = shape[:2]
    g = len(wls)
    _, out_win = _windows(name)
    rng = np.random.default_rng(6100 + n + c)
    x = (2 * rng.random(shape, dtype=np.float32) - 0.5).astype(np.float32)
    x.reshape(-1)[:: 97] = np.float32(TAU)
    x.reshape(-1)[1:: 89] = np.float32(0.0)
    x.reshape(-1)[2:: 83] = np.float32(1.0)
    target = rng.random((b, g) + out_win[2:], dtype=np.float32)
    w = ((2 * rng.random((b, c) + out_win[2:], dtype=np.float32) - 1)
         + 1j * (2 * rng.random((b, c) + out_win[2:], dtype=np.float32) - 1)).astype(np.complex64)
    gi = (2 * rng.random((b, g) + out_win[2:], dtype=np.float32) - 1).astype(np.float32)
    hs = tuple(O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, wl, Z, O.TF_ASM) for wl in wls)
    for a in (x, target, w, gi) + hs:
        a.setflags(write=False)
    return x, target, w, gi, hs


def _field_of(name, threshold, field):
    """u float64 [B, C, N, N]: the embedded leaf, binarised inside its window with a threshold"""
    n = CASES[name][0]
    x = _case(name)[0]
    u = binarize(x, TAU, FIELD[field]) if threshold else x
    return embed(u.astype(np.float64), _windows(name)[0], n)


@functools.lru_cache(maxsize=None)
def _oracle(name, threshold, field):
    """the float64 field [B, G, P, h_o, w_o] and intensity [B, G, h_o, w_o] over the roi"""
    n, shape, wls, _, _ = CASES[name]
    b, c = shape[:2]
    g = len(wls)
    hs = _case(name)[4]
    u = _field_of(name, threshold, field).reshape(b, g, c // g, n, n)
    fld = np.stack([np.stack([O.propagate(u[e, k], hs[k]) for k in range(g)]) for e in range(b)])
    fld = np.ascontiguousarray(crop(fld, _windows(name)[1]))
    inten = np.mean(fld.real ** 2 + fld.imag ** 2, axis=2)
    return fld, inten


def _pull_back(name, g_out, threshold, field):
    """crop_in Re A(-z)[embed_out g_out], times vb s(x) under the default STE gate: g_out complex
    [B, G, P, h_o, w_o] = dL/dF over the roi -> float64, the leaf's shape"""
    n, shape, wls, _, _ = CASES[name]
    in_win, out_win = _windows(name)
    x, hs = _case(name)[0], _case(name)[4]
    full = embed(g_out, out_win, n)
    back = np.stack([np.stack([O.propagate(full[e, k], np.conj(hs[k])) for k in range(len(wls))])
                     for e in range(shape[0])])
    grad = crop(back.real, in_win).reshape(shape)
    if threshold:
        grad = field_values(FIELD[field])[1] * ste_surrogate(x, STE_WINDOW, 0.0, 1.0) * grad
    return grad


def _leaf(name, dtype=torch.float32):
    return torch.from_numpy(_case(name)[0].copy()).to(dtype).cuda().requires_grad_()


def _check_gradient(label, x, want):
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.dtype == x.dtype and tuple(x.grad.shape) == tuple(x.shape)
    got = x.grad.cpu().numpy().astype(np.float64)
    scale = np.max(np.abs(want))
    e = np.max(np.abs(got - want)) / scale
    print(f"{label}: grad err {e:.3e} of max|want| = {scale:.3e}")
    assert scale > 0.0 and e <= FIELD_RTOL


MODES = [(False, "amplitude"), (True, "amplitude"), (True, "phase")]


def _mode_kw(threshold, field):
    return {"field": field, **({"threshold": TAU} if threshold else {})}


# -- simulate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold, field", MODES)
@pytest.mark.parametrize("name", ["mono", "centred256"])
def test_simulate_window(name, threshold, field):
    import torch.nn.functional as F
    import torchOptics.optics as tt
    n, shape, wls, _, _ = CASES[name]
    in_win, out_win = _windows(name)
    x_np, _, w_np, _, _ = _case(name)
    meta = _meta(wls)
    kw = dict(_kw(name), binary=False, **_mode_kw(threshold, field))
    xr = _leaf(name)
    plain = tt.simulate(tt.Tensor(torch.from_numpy(x_np.copy()).cuda(), meta=meta), Z, **kw)
    graph = tt.simulate(tt.Tensor(xr, meta=meta), Z, **kw)
    assert plain.dtype == torch.complex64 and tuple(plain.shape) == shape[:2] + out_win[2:]
    assert plain.grad_fn is None and graph.grad_fn is not None
    assert torch.equal(torch.view_as_real(graph.detach()), torch.view_as_real(plain))
    # the route it replaces: the embedded field through the unwindowed call, sliced
    u = torch.from_numpy(_field_of(name, threshold, field).astype(np.float32)).cuda()
    y0, x0, h, w = in_win
    assert torch.equal(u, F.pad(crop(u, in_win), (x0, n - x0 - w, y0, n - y0 - h)))
    full = tt.simulate(tt.Tensor(u, meta=meta), Z, binary=False)
    assert torch.equal(torch.view_as_real(plain), torch.view_as_real(crop(full, out_win).contiguous()))
    want_f = _oracle(name, threshold, field)[0].reshape(plain.shape)
    e = np.max(np.abs(plain.cpu().numpy() - want_f)) / float(full.abs().max())   # max|field| over the grid
    print(f"simulate {name} thr={threshold} {field}: field err {e:.3e} of max|field|")
    assert e <= FIELD_RTOL
    wt = torch.from_numpy(w_np.copy()).cuda()
    (torch.view_as_real(graph) * torch.view_as_real(wt)).sum().backward()
    b, c = shape[:2]
    g_out = w_np.astype(np.complex128).reshape((b, 1, c) + out_win[2:])
    _check_gradient(f"simulate {name} thr={threshold} {field}", xr, _pull_back(name, g_out, threshold, field))


def test_simulate_window_pads_an_odd_plane_count():
    import torchOptics.optics as tt
    x = torch.rand((1, 3, 20, 31), device="cuda")
    both = tt.simulate(tt.Tensor(x, meta=_meta((WL,))), Z, binary=False, grid=64, threshold=TAU, field="phase")
    pair = tt.simulate(tt.Tensor(x[:, :2].contiguous(), meta=_meta((WL,))), Z, binary=False, grid=64, threshold=TAU,
                       field="phase")
    assert tuple(both.shape) == (1, 3, 20, 31)
    assert torch.equal(torch.view_as_real(both[:, :2].contiguous()), torch.view_as_real(pair))


# -- intensity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold, field", MODES)
@pytest.mark.parametrize("name", ["mono", "rgb"])
def test_intensity_window(name, threshold, field):
    import torchOptics.optics as tt
    n, shape, wls, _, _ = CASES[name]
    _, out_win = _windows(name)
    x_np, _, _, gi_np, _ = _case(name)
    fld64, inten64 = _oracle(name, threshold, field)
    meta = _meta(wls)
    kw = dict(_kw(name), **_mode_kw(threshold, field))
    plain = tt.intensity(tt.Tensor(torch.from_numpy(x_np.copy()).cuda(), meta=meta), Z, **kw)
    xr = _leaf(name)
    graph = tt.intensity(tt.Tensor(xr, meta=meta), Z, **kw)
    assert tuple(plain.shape) == inten64.shape and plain.grad_fn is None and graph.grad_fn is not None
    assert torch.equal(graph.detach(), plain)
    u = torch.from_numpy(_field_of(name, threshold, field).astype(np.float32)).cuda()
    full = tt.intensity(tt.Tensor(u, meta=meta), Z)
    assert torch.equal(plain, crop(full, out_win).contiguous())
    e = np.max(np.abs(plain.cpu().numpy() - inten64)) / np.max(np.abs(full.cpu().numpy()))
    print(f"intensity {name} thr={threshold} {field}: err {e:.3e} of max I")
    assert e <= FIELD_RTOL
    (graph * torch.from_numpy(gi_np.copy()).cuda()).sum().backward()
    p = shape[1] // len(wls)
    g_out = (2.0 / p) * gi_np.astype(np.float64)[:, :, None] * fld64
    _check_gradient(f"intensity {name} thr={threshold} {field}", xr, _pull_back(name, g_out, threshold, field))


# -- loss ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["mse", "psnr"])
@pytest.mark.parametrize("threshold, field", MODES)
@pytest.mark.parametrize("name", ["mono", "rgb"])
def test_loss_window(name, threshold, field, metric):
    import torchOptics.optics as tt
    n, shape, wls, _, _ = CASES[name]
    _, out_win = _windows(name)
    b, g = shape[0], len(wls)
    x_np, t_np, _, _, _ = _case(name)
    fld64, inten64 = _oracle(name, threshold, field)
    kind = LOSS_PSNR if metric == "psnr" else LOSS_MSE
    count = g * out_win[2] * out_win[3]
    meta = _meta(wls)
    kw = dict(_kw(name), metric=metric, **_mode_kw(threshold, field))
    tgt = torch.from_numpy(t_np.copy()).cuda()
    plain = tt.loss(tt.Tensor(torch.from_numpy(x_np.copy()).cuda(), meta=meta), tgt, Z, **kw)
    xr = _leaf(name)
    graph = tt.loss(tt.Tensor(xr, meta=meta), tgt, Z, **kw)
    torch.cuda.synchronize()
    assert plain.dtype == torch.float64 and tuple(plain.shape) == (b,) and graph.grad_fn is not None
    assert torch.equal(graph.detach(), plain)
    up = UP[:b]
    want_g = np.empty_like(fld64)
    for e in range(b):
        stats = np.stack([O.chan_stats(inten64[e, k], t_np[e, k].astype(np.float64)) for k in range(g)])
        if metric == "psnr":
            want = O.psnr_from_stats(stats, count)
            err = abs(float(plain[e]) - want)
            assert err <= PSNR_ATOL
        else:
            s = stats.sum(0)
            want = (s[2] - s[0] * s[0] / s[1]) / count
            err = abs(float(plain[e]) - want) / want
            assert err <= MSE_RTOL
        print(f"loss {name} thr={threshold} {field} {metric} env {e}: {float(plain[e]):.9g} oracle {want:.9g} err {err:.3e}")
        a, c = loss_coeffs(stats, kind, REL_LSQ, count, up[e])
        wgt = a * inten64[e] + c * t_np[e].astype(np.float64)
        want_g[e] = (2.0 / (shape[1] // g)) * wgt[:, None] * fld64[e]
    (graph * torch.from_numpy(up.copy()).cuda()).sum().backward()
    _check_gradient(f"loss {name} thr={threshold} {field} {metric}", xr, _pull_back(name, want_g, threshold, field))


# -- end to end ----------------------------------------------------------------------------------------
def test_adam_through_a_windowed_binary_loss_lowers_it():
    """Sixteen Adam steps on logits through tt.loss(sigmoid(logits), threshold=0.5, grid=64, roi=..) on a
    40 x 33 leaf; Plan.evaluate_threshold_window on the final leaf gives the last forward value bit for bit."""
    import hbx
    import torchOptics.optics as tt
    from hbx import _lib
    rng = np.random.default_rng(45)
    c, h, w = 4, 40, 33
    origin, roi = (5, 9), (3, 20, 50, 31)
    logits = torch.from_numpy(rng.standard_normal((1, c, h, w)).astype(np.float32)).cuda().requires_grad_()
    target = torch.from_numpy(rng.random((1, 1) + roi[2:], dtype=np.float32)).cuda()
    meta = _meta((WL,))
    kw = dict(threshold=0.5, grid=64, origin=origin, roi=roi)
    opt = torch.optim.Adam([logits], lr=0.1)
    losses = []
    for _ in range(16):
        opt.zero_grad()
        val = tt.loss(tt.Tensor(torch.sigmoid(logits), meta=meta), target, Z, **kw).sum()
        val.backward()
        opt.step()
        losses.append(val.detach())
    with torch.no_grad():
        x = torch.sigmoid(logits)
        last = tt.loss(tt.Tensor(x, meta=meta), target, Z, **kw)
    graph = tt.loss(tt.Tensor(torch.sigmoid(logits), meta=meta), target, Z, **kw)
    plan = hbx.Plan(hbx.OpticsConfig(64, 64, 1, c, (WL,), O.PIXEL_PITCH, O.PIXEL_PITCH, Z), max_jobs=1)
    _, _, stats, _ = plan.evaluate_threshold_window(x, 0.5, origin + (h, w), target, roi, want_field=False,
                                                    want_intensity=False)
    direct = plan.loss_window(stats, roi, _lib.LOSS_MSE, _lib.REL_LSQ)
    losses = [float(v) for v in losses]
    print("windowed binary losses", " ".join(f"{v:.6f}" for v in losses), "final", float(last[0]))
    assert float(last[0]) < losses[0]
    assert torch.equal(last, direct) and torch.equal(graph.detach(), direct)
    plan.close()
