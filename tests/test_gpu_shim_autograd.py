"""Gradients through tt.simulate(.., binary=False).

The forward is A u = IFFT2(FFT2(u) H(z)); the backward pass runs hbx_simulate_complex on the plan
for -z (H(-z) = conj H(z) exactly, tests/test_complex_field_host.py), which is A^H.  For the loss
L = sum w (Re F^2 + Im F^2) the gradient that reaches the propagation is g = 2 w F, so x.grad is
compared with the oracle's adjoint O.propagate(g, conj h) of the g that the downloaded GPU field
implies (float64): one propagation separates the two sides, so the single-propagation tolerance
FIELD_RTOL x max|want| applies.  A real leaf takes the real part, a complex leaf the whole field,
and a phase leaf (u = exp(i pi x)) Re(conj(du/dx) A^H g) with du/dx = i pi u, torch's rule for a
real input of a complex function."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

Z = 2e-3
WL = 515e-9
META = {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": WL}
FIELD_RTOL = 2e-5


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _h(n, tf_kind=O.TF_ASM):
    return O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, WL, Z, tf_kind)


def _leaf(shape, seed, complex_leaf=False, dtype=np.float32):
    rng = np.random.default_rng(seed)
    a = (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)
    if complex_leaf:
        b = (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)
        a = (a + 1j * b).astype(np.complex64)
    else:
        a = a.astype(dtype)
    return a


CASES = {
    # name: (shape, complex leaf, simulate keywords, oracle tf kind, phase)
    "real_asm": ((2, 4, 64, 64), False, {}, O.TF_ASM, False),
    "real_fresnel": ((2, 4, 64, 64), False, {"tf": "fresnel"}, O.TF_FRESNEL, False),
    "complex": ((2, 3, 64, 64), True, {}, O.TF_ASM, False),
    "phase": ((1, 4, 64, 64), False, {"field": "phase"}, O.TF_ASM, True),
    "odd_planes_chw": ((3, 64, 64), False, {}, O.TF_ASM, False),
    "real_256": ((1, 2, 256, 256), False, {}, O.TF_ASM, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_is_the_oracle_adjoint(name):
    import torchOptics.optics as tt
    shape, complex_leaf, kw, tf_kind, phase = CASES[name]
    n = shape[-1]
    x_np = _leaf(shape, 40 + len(name), complex_leaf)
    w_np = np.random.default_rng(7).random(shape, dtype=np.float32)
    x = torch.from_numpy(x_np).cuda().requires_grad_()
    w = torch.from_numpy(w_np).cuda()
    F = tt.simulate(tt.Tensor(x, meta=META), Z, binary=False, **kw)
    assert F.grad_fn is not None and F.dtype == torch.complex64 and tuple(F.shape) == shape
    L = (w * (F.real ** 2 + F.imag ** 2)).sum()
    L.backward()
    torch.cuda.synchronize()

    h = _h(n, tf_kind)
    x64 = x_np.astype(np.complex128 if complex_leaf else np.float64)
    u64 = np.exp(1j * np.pi * x64) if phase else x64
    want_f = O.propagate(u64, h)
    f_gpu = F.detach().cpu().numpy().astype(np.complex128)
    ef = np.max(np.abs(f_gpu - want_f)) / np.max(np.abs(want_f))

    g = 2.0 * w_np.astype(np.float64) * f_gpu          # dL/dF as torch hands it to the backward pass
    adj = O.propagate(g, np.conj(h))
    if phase:
        want_g = (np.conj(1j * np.pi * u64) * adj).real
    elif complex_leaf:
        want_g = adj
    else:
        want_g = adj.real
    assert x.grad is not None
    assert x.grad.dtype == x.dtype and tuple(x.grad.shape) == shape
    eg = np.max(np.abs(x.grad.cpu().numpy() - want_g)) / np.max(np.abs(want_g))
    print(f"{name}: field err {ef:.3e} of max|want|, grad err {eg:.3e} of max|want|")
    assert ef <= FIELD_RTOL
    assert eg <= FIELD_RTOL


@pytest.mark.parametrize("complex_leaf", [False, True])
def test_gradient_of_a_loss_that_ends_in_conj(complex_leaf):
    """L = |sum conj(F) T|^2 (an overlap with a target field): torch hands the backward pass a
    lazily conjugated grad_output (is_conj), whose memory holds the unconjugated values; the
    shim must propagate the gradient itself.  With S = sum conj(F) T the gradient that reaches
    the propagation is g = 2 conj(S) T, formed here in float64 from the downloaded field."""
    import torchOptics.optics as tt
    shape = (1, 2, 64, 64)
    x_np = _leaf(shape, 61, complex_leaf)
    t_np = _leaf(shape, 62, True)
    x = torch.from_numpy(x_np).cuda().requires_grad_()
    target = torch.from_numpy(t_np).cuda()
    F = tt.simulate(tt.Tensor(x, meta=META), Z, binary=False)
    s = (F.conj() * target).sum()
    (s.real ** 2 + s.imag ** 2).backward()
    torch.cuda.synchronize()
    h = _h(64)
    f_gpu = F.detach().cpu().numpy().astype(np.complex128)
    t64 = t_np.astype(np.complex128)
    g = 2.0 * np.conj(np.sum(np.conj(f_gpu) * t64)) * t64
    adj = O.propagate(g, np.conj(h))
    want_g = adj if complex_leaf else adj.real
    assert x.grad.dtype == x.dtype and tuple(x.grad.shape) == shape
    eg = np.max(np.abs(x.grad.cpu().numpy() - want_g)) / np.max(np.abs(want_g))
    # the wrong answer (conj(g) propagated) for scale
    bad = O.propagate(np.conj(g), np.conj(h))
    eb = np.max(np.abs((bad if complex_leaf else bad.real) - want_g)) / np.max(np.abs(want_g))
    print(f"complex_leaf={complex_leaf}: grad err {eg:.3e} of max|want| (conj(g) would give {eb:.3e})")
    assert eb > 100 * FIELD_RTOL              # the case can tell the two apart
    assert eg <= FIELD_RTOL


def test_lazily_conjugated_input_is_propagated_conjugated():
    """x.conj() is a view with the conjugate bit set over x's memory: simulate must see conj(x)."""
    import torchOptics.optics as tt
    x_np = _leaf((2, 4, 64, 64), 63, True)
    x = torch.from_numpy(x_np).cuda()
    xc = x.conj()
    assert xc.is_conj()
    got = tt.simulate(tt.Tensor(xc, meta=META), Z, binary=False).cpu().numpy()
    want = O.propagate(np.conj(x_np.astype(np.complex128)), _h(64))
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"conj input: field err {err:.3e} of max|want|")
    assert err <= FIELD_RTOL
    # a lazily negated real view (the imaginary part of a conjugated tensor) on the real route
    xi = xc.imag
    assert xi.is_neg()
    got = tt.simulate(tt.Tensor(xi, meta=META), Z, binary=False).cpu().numpy()
    want = O.propagate(-x_np.imag.astype(np.float64), _h(64))
    assert np.max(np.abs(got - want)) <= FIELD_RTOL * np.max(np.abs(want))


def test_float64_leaf_gets_a_float64_gradient():
    import torchOptics.optics as tt
    x_np = _leaf((1, 2, 64, 64), 51, dtype=np.float64)
    x = torch.from_numpy(x_np).cuda().requires_grad_()
    F = tt.simulate(tt.Tensor(x, meta=META), Z, binary=False)
    (F.real ** 2 + F.imag ** 2).sum().backward()
    assert x.grad.dtype == torch.float64 and tuple(x.grad.shape) == (1, 2, 64, 64)
    # sum |A u|^2 = sum |u|^2 below the evanescent cut, so the gradient is close to 2 u
    f_gpu = F.detach().cpu().numpy().astype(np.complex128)
    want = O.propagate(2.0 * f_gpu, np.conj(_h(64))).real
    assert np.max(np.abs(x.grad.cpu().numpy() - want)) <= FIELD_RTOL * np.max(np.abs(want))


def test_no_graph_without_a_gradient_request():
    import torchOptics.optics as tt
    x = torch.from_numpy(_leaf((1, 2, 64, 64), 52)).cuda()
    assert tt.simulate(tt.Tensor(x, meta=META), Z, binary=False).grad_fn is None
    xr = x.clone().requires_grad_()
    with torch.no_grad():
        out = tt.simulate(tt.Tensor(xr, meta=META), Z, binary=False)
    assert out.grad_fn is None and not out.requires_grad
    # and the values are those of the differentiable call, bit for bit
    out_g = tt.simulate(tt.Tensor(xr, meta=META), Z, binary=False)
    assert out_g.grad_fn is not None
    assert torch.equal(torch.view_as_real(out_g.detach()), torch.view_as_real(out))


def test_binary_path_builds_no_graph():
    import torchOptics.optics as tt
    m = (np.random.default_rng(53).random((1, 2, 64, 64)) >= 0.5).astype(np.float32)
    x = torch.from_numpy(m).cuda().requires_grad_()
    out = tt.simulate(tt.Tensor(x, meta=META), Z, strict=True)
    assert out.grad_fn is None and not out.requires_grad


def test_gradient_descent_lowers_the_loss():
    """Ten steps of plain gradient descent on mse(mean_p |F_p|^2, target) from a fixed seed: the
    step size 500 is well inside 2 / L of this loss (its gradient is Lipschitz with L about
    2 (2 max|F| / P)^2 / N^2 = 3e-4 at N = 64, P = 4), so every step lowers it."""
    import torch.nn.functional as Fn
    import torchOptics.optics as tt
    rng = np.random.default_rng(31)
    x = torch.from_numpy(rng.random((1, 4, 64, 64), dtype=np.float32)).cuda().requires_grad_()
    target = torch.from_numpy(rng.random((1, 64, 64), dtype=np.float32)).cuda()
    losses = []
    for _ in range(10):
        F = tt.simulate(tt.Tensor(x, meta=META), Z, binary=False)
        loss = Fn.mse_loss((F.real ** 2 + F.imag ** 2).mean(dim=1), target)
        x.grad = None
        loss.backward()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            x -= 500.0 * x.grad
    print("losses", " ".join(f"{v:.6f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert losses[-1] < losses[0]
