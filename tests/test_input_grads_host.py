"""Input-gradient entry points of the C ABI (gd_psf_to_otf_backward, gd_conv_fft_batch_backward_otf,
gd_admm_train_full_saved_bytes, gd_admm_train_iter_full, gd_admm_train_iter_full_backward) and
``DifferentiableUnrolledADMM``: declarations, the saved footprint, argument validation and the module's host-side
contract.  Host only: every engine call here returns before any HIP call."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

GAUSS, POIS = 0, 1
NAMES = ("gd_psf_to_otf_backward", "gd_conv_fft_batch_backward_otf", "gd_admm_train_full_saved_bytes",
         "gd_admm_train_iter_full", "gd_admm_train_iter_full_backward")


@pytest.fixture(scope="module")
def lib():
    from gdeconv import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("ge", os.path.join(ROOT, "__graft_entry__.py"))
        ge = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ge)
        ge.build()
    return _lib.load()


def test_header_declares_and_binding_lists_the_entry_points(lib):
    from gdeconv import _lib
    with open(os.path.join(ROOT, "include", "gdeconv.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.gd_abi_version() == 5          # purely additive
    assert "OTF-GRADIENT CONVENTION" in header


def test_full_saved_bytes_is_two_half_spectra_and_one_image(lib):
    """Documented in include/gdeconv.h: X and F(w), 2 x N (W/2+1) H 8 bytes, plus one image (vt; x when last)."""
    f = lib.gd_admm_train_full_saved_bytes
    N, L = 3, 48
    spec, img = N * 25 * L * 8, N * L * L * 4
    assert f(N, L, L) == 2 * spec + img
    assert f(N, L, L) == lib.gd_admm_train_saved_bytes(N, L, L) + spec     # one half spectrum more than the plain body
    assert f(3, 33, 45) == 2 * 3 * 23 * 33 * 8 + 3 * 33 * 45 * 4
    assert f(3, 4097, 48) == 0 and f(3, 48, 1) == 0                        # unsupported sizes
    assert f(0, 48, 48) == 0


def _bufs(n):
    """n distinct non-NULL host addresses (never dereferenced: validation returns first)."""
    keep = [ctypes.c_float(0.0) for _ in range(n)]
    return keep, [ctypes.addressof(k) for k in keep]


def _iter(lib, p, llh=POIS, last=0, L=48, N=3, **over):
    a = dict(y=p[0], z=p[1], u1=p[2], w=p[3], alpha=p[4], rho1=p[5], rho2=p[6], rho2n=p[7], otf=p[8], zin=p[9],
             u1o=p[10], wo=p[11], saved=p[12], ws=p[13])
    a.update(over)
    return lib.gd_admm_train_iter_full(a["y"], a["z"], a["u1"], a["w"], a["alpha"], 0, a["rho1"], 0, a["rho2"], 0,
                                       a["rho2n"], 0, llh, last, N, L, L, a["otf"], a["zin"], a["u1o"], a["wo"],
                                       a["saved"], a["ws"], None)


def _bwd(lib, p, llh=POIS, last=0, L=48, N=3, **over):
    a = dict(gzin=p[0], gu1o=p[1], gwo=p[2], y=p[3], alpha=p[4], rho1=p[5], rho2=p[6], rho2n=p[7], otf=p[8],
             saved=p[9], gz=p[10], gu1=p[11], gw=p[12], part=p[13], gotf=p[14], gy=p[15], apart=p[16], ws=p[17])
    a.update(over)
    return lib.gd_admm_train_iter_full_backward(
        a["gzin"], a["gu1o"], a["gwo"], a["y"], a["alpha"], 0, a["rho1"], 0, a["rho2"], 0, a["rho2n"], 0, llh, last,
        N, L, L, a["otf"], a["saved"], a["gz"], a["gu1"], a["gw"], a["part"], a["gotf"], a["gy"], a["apart"], a["ws"],
        None)


def test_body_argument_errors_need_no_device(lib):
    keep, p = _bufs(18)
    assert _iter(lib, p, llh=2) == -1 and _bwd(lib, p, llh=-1) == -1
    assert b"llh" in lib.gd_last_error()
    # aliasing between outputs and inputs, or between two outputs
    assert _iter(lib, p, u1o=p[2]) == -1
    assert b"alias" in lib.gd_last_error()
    assert _iter(lib, p, zin=p[1]) == -1 and _iter(lib, p, wo=p[3]) == -1 and _iter(lib, p, saved=p[8]) == -1
    assert _iter(lib, p, u1o=p[9]) == -1
    assert _bwd(lib, p, gz=p[0]) == -1 and _bwd(lib, p, gy=p[3]) == -1 and _bwd(lib, p, gotf=p[8]) == -1
    assert _bwd(lib, p, gotf=p[9]) == -1                 # the OTF gradient over the saved spectra
    assert _bwd(lib, p, gy=p[12]) == -1                  # g_y == g_w
    assert _bwd(lib, p, apart=p[13]) == -1               # the alpha parts over the rho parts
    # NULL outputs and required pointers
    for k in ("gotf", "gy", "apart", "gz", "part"):
        assert _bwd(lib, p, **{k: None}) == -1, k
    assert _iter(lib, p, saved=None) == -1 and _iter(lib, p, rho2n=None) == -1
    assert _bwd(lib, p, gu1o=None) == -1 and _bwd(lib, p, rho2n=None) == -1   # not last: both are read
    # unsupported side
    assert _iter(lib, p, L=4097) == -2 and _bwd(lib, p, L=4097) == -2
    # an empty batch is valid and launches nothing
    assert _iter(lib, p, N=0) == 0 and _bwd(lib, p, N=0) == 0
    del keep


def test_adjoint_argument_errors_need_no_device(lib):
    keep, p = _bufs(4)
    f, c = lib.gd_psf_to_otf_backward, lib.gd_conv_fft_batch_backward_otf
    assert f(p[0], 47, 47, 3, 48, 48, p[1], p[2], None) == -1            # odd PSF
    assert b"even" in lib.gd_last_error()
    assert f(p[0], 64, 64, 3, 48, 48, p[1], p[2], None) == -1            # PSF larger than the image
    assert f(p[0], 16, 16, 3, 4097, 48, p[1], p[2], None) == -2          # unsupported size
    assert f(p[0], 16, 16, 3, 48, 48, None, p[2], None) == -1            # NULL output
    assert f(None, 16, 16, 3, 48, 48, p[1], p[2], None) == -1
    assert f(p[0], 16, 16, 3, 48, 48, p[0], p[2], None) == -1            # output over its input
    assert f(p[0], 16, 16, 0, 48, 48, p[1], p[2], None) == 0             # empty batch
    assert c(p[0], p[1], 0, 3, 48, 4097, p[2], p[3], None) == -2
    assert c(p[0], p[1], 0, 3, 48, 48, None, p[3], None) == -1
    assert c(p[0], p[1], 1, 3, 48, 48, p[0], p[3], None) == -1           # the OTF gradient over x
    assert c(p[0], p[1], 1, 3, 48, 48, p[1], p[3], None) == -1           # ... over g_out
    assert b"alias" in lib.gd_last_error()
    assert c(p[0], p[1], 0, 0, 48, 48, p[2], p[3], None) == 0
    del keep


@pytest.mark.parametrize("subnet", [True, False])
def test_keys_equal_the_inference_class(subnet):
    from gdeconv.models import DifferentiableUnrolledADMM, TrainableUnrolledADMM, Unrolled_ADMM
    a = Unrolled_ADMM(n_iters=3, llh="Poisson", subnet=subnet)
    b = DifferentiableUnrolledADMM(n_iters=3, llh="Poisson", subnet=subnet)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert isinstance(b, TrainableUnrolledADMM) and isinstance(b, Unrolled_ADMM)
    b.load_state_dict(a.state_dict())          # checkpoints move both ways
    a.load_state_dict(b.state_dict())
    for k in ("n", "llh", "PnP", "subnet", "denoiser"):
        assert getattr(a, k) == getattr(b, k)


def test_class_is_exported():
    import gdeconv.models as M
    assert "DifferentiableUnrolledADMM" in M.__all__
    from models.Unrolled_ADMM import DifferentiableUnrolledADMM
    assert DifferentiableUnrolledADMM is M.DifferentiableUnrolledADMM
    assert "DifferentiableUnrolledADMM" in M.__doc__


@pytest.mark.parametrize("which", [None, 0, 1, 2])
def test_rejects_cpu_tensors(which):
    from gdeconv.models import DifferentiableUnrolledADMM
    m = DifferentiableUnrolledADMM(n_iters=2, llh="Gaussian", subnet=False)
    m.Z = torch.nn.Identity()
    ins = [torch.rand(2, 1, 32, 32), torch.rand(2, 1, 16, 16), torch.ones(2, 1, 1, 1)]
    if which is not None:
        ins[which].requires_grad_()
    with pytest.raises(ValueError, match="ROCm"):
        m(*ins)


def test_differentiable_entry_points_reject_cpu_tensors():
    from gdeconv import engine
    with pytest.raises(ValueError, match="ROCm"):
        engine.psf_to_otf_half(torch.rand(2, 1, 16, 16, requires_grad=True), 2, 32, 32)
    with pytest.raises(ValueError, match="ROCm"):
        engine.conv_half(torch.zeros(2, 17, 32, dtype=torch.complex64), torch.rand(2, 1, 32, 32, requires_grad=True))
