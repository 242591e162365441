"""tt.simulate on continuous fields (binary=False) and the tf / field / rel_scale switches of the
shim, against the float64 oracle at N = 64.  Tolerances are tests/test_gpu_parity.py's: field
<= 2e-5 max|want|, PSNR <= 1e-4 dB.  Inputs are float32 / complex64 draws handed to the oracle
as their float64 / complex128 upcast."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

N = 64
Z = 2e-3
WL = 515e-9
META = {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": WL}
FIELD_RTOL = 2e-5
PSNR_TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _h(tf_kind=O.TF_ASM):
    return O.transfer_function(N, N, O.PIXEL_PITCH, O.PIXEL_PITCH, WL, Z, tf_kind)


def _close(got: torch.Tensor, want: np.ndarray):
    assert got.dtype == torch.complex64 and tuple(got.shape) == want.shape
    err = np.max(np.abs(got.cpu().numpy() - want))
    assert err <= FIELD_RTOL * np.max(np.abs(want)), err / np.max(np.abs(want))


@pytest.mark.parametrize("planes", [8, 3])
def test_continuous_real_field(planes):
    import torchOptics.optics as tt
    x = np.random.default_rng(planes).random((2, planes, N, N), dtype=np.float32)
    got = tt.simulate(tt.Tensor(torch.from_numpy(x), meta=META), Z, binary=False)
    _close(got, O.propagate(x.astype(np.float64), _h()))
    # [C, H, W] input, float64 samples (cast to float32), and an input already on the GPU
    got3 = tt.simulate(tt.Tensor(torch.from_numpy(x[0].astype(np.float64)).cuda(), meta=META), Z, binary=False)
    _close(got3, O.propagate(x[0].astype(np.float64), _h()))


def test_continuous_complex_field():
    import torchOptics.optics as tt
    rng = np.random.default_rng(21)
    a = (2 * rng.random((2, 3, N, N), dtype=np.float32) - 1).astype(np.float32)
    b = (2 * rng.random((2, 3, N, N), dtype=np.float32) - 1).astype(np.float32)
    x = torch.complex(torch.from_numpy(a), torch.from_numpy(b))
    got = tt.simulate(tt.Tensor(x, meta=META), Z, binary=False)
    _close(got, O.propagate(a.astype(np.float64) + 1j * b.astype(np.float64), _h()))
    with pytest.raises(ValueError):
        tt.simulate(tt.Tensor(x, meta=META), Z)                               # binary path: refused
    with pytest.raises(ValueError):
        tt.simulate(tt.Tensor(x, meta=META), Z, binary=False, field="phase")  # a complex field is the field


def test_continuous_phase_field():
    import torchOptics.optics as tt
    x = np.random.default_rng(22).random((1, 4, N, N), dtype=np.float32)
    got = tt.simulate(tt.Tensor(torch.from_numpy(x), meta=META), Z, binary=False, field="phase")
    _close(got, O.propagate(np.exp(1j * np.pi * x.astype(np.float64)), _h()))


@pytest.mark.parametrize("kw,tf_kind,field_kind", [({"tf": "fresnel"}, O.TF_FRESNEL, O.FIELD_AMPLITUDE),
                                                   ({"field": "phase"}, O.TF_ASM, O.FIELD_PHASE),
                                                   ({"tf": O.TF_FRESNEL, "field": O.FIELD_PHASE}, O.TF_FRESNEL,
                                                    O.FIELD_PHASE)])
def test_binary_mask_switches(kw, tf_kind, field_kind):
    import torchOptics.optics as tt
    m = (np.random.default_rng(23).random((1, 4, N, N)) >= 0.5).astype(np.int8)
    got = tt.simulate(tt.Tensor(m, meta=META), Z, strict=True, **kw)
    _close(got, O.propagate(O.mask_to_field(m, field_kind), _h(tf_kind)))
    # the default call on the same mask is still ASM / amplitude (the switches are part of the plan key)
    _close(tt.simulate(tt.Tensor(m, meta=META), Z, strict=True), O.propagate(O.mask_to_field(m), _h()))


def test_relative_loss_rel_scale_none_gpu_and_cpu():
    import torchOptics.metrics as tm
    import torchOptics.optics as tt
    rng = np.random.default_rng(24)
    x = rng.random((3, N, N), dtype=np.float32)
    y = rng.random((3, N, N), dtype=np.float32)
    want_none = O.relative_psnr(x, y, rel_scale=O.REL_NONE)
    want_lsq = O.relative_psnr(x, y, rel_scale=O.REL_LSQ)
    assert abs(want_none - want_lsq) > 1e-2          # the two scales differ on this data
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    assert abs(tt.relativeLoss(xg, yg, tm.get_PSNR, rel_scale="none") - want_none) <= PSNR_TOL   # hbx_rel_stats
    assert abs(tt.relativeLoss(xg, yg, tm.get_PSNR, rel_scale=O.REL_NONE) - want_none) <= PSNR_TOL
    assert abs(tt.relativeLoss(xg, yg, tm.get_PSNR) - want_lsq) <= PSNR_TOL
    xc, yc = torch.from_numpy(x), torch.from_numpy(y)                                            # torch fallback
    assert abs(tt.relativeLoss(xc, yc, tm.get_PSNR, rel_scale="none") - want_none) <= PSNR_TOL
    assert abs(tt.relativeLoss(xc, yc, tm.get_PSNR) - want_lsq) <= PSNR_TOL


def test_continuous_call_leaves_the_binary_check_alone():
    import torchOptics.optics as tt
    x = tt.Tensor(np.full((1, 2, N, N), 0.5, np.float32), meta=META)
    tt.check_binary()                                   # nothing pending from earlier tests
    tt.simulate(x, Z, binary=False)
    tt.simulate(x, Z, binary=False, strict=True)        # strict has nothing to check here
    tt.check_binary()                                   # does not raise
    with pytest.raises(ValueError):
        tt.simulate(x, Z, strict=True)                  # the default call on the same data still does
    tt.check_binary()
