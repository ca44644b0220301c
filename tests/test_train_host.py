"""Training entry points of the C ABI (gd_admm_train_*) and ``TrainableUnrolledADMM``: declarations, the saved
footprint, argument validation and the module's host-side contract.  Host only: every engine call here returns
before any HIP call."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

GAUSS, POIS = 0, 1
NAMES = ("gd_admm_train_saved_bytes", "gd_admm_train_init", "gd_admm_train_iter", "gd_admm_train_iter_backward")


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


def test_saved_bytes_is_one_half_spectrum_and_one_image(lib):
    """Documented in include/gdeconv.h: k x N (W/2+1) H 8 bytes with k = 1 (E = conj(H) W - X), plus one image (vt)."""
    f = lib.gd_admm_train_saved_bytes
    N, L = 3, 48
    spec, img = N * 25 * L * 8, N * L * L * 4
    b = f(N, L, L)
    assert b > 0
    assert (b - img) > 0 and (b - img) % spec == 0       # a positive multiple of the half spectrum, plus the image
    assert b <= 2 * spec + img
    assert b == spec + img
    assert f(3, 33, 45) == 3 * 23 * 33 * 8 + 3 * 33 * 45 * 4
    assert f(3, 4097, 48) == 0 and f(3, 48, 1) == 0      # unsupported sizes
    assert f(0, 48, 48) == 0


def _bufs(n):
    """n distinct non-NULL host addresses (never dereferenced: validation returns first)."""
    keep = [ctypes.c_float(0.0) for _ in range(n)]
    return keep, [ctypes.addressof(k) for k in keep]


def _iter(lib, p, llh=POIS, last=0, L=48, **over):
    a = dict(y=p[0], z=p[1], u1=p[2], w=p[3], alpha=p[4], rho1=p[5], rho2=p[6], rho2n=p[7], otf=p[8], zin=p[9],
             u1o=p[10], wo=p[11], saved=p[12], ws=p[13])
    a.update(over)
    return lib.gd_admm_train_iter(a["y"], a["z"], a["u1"], a["w"], a["alpha"], 0, a["rho1"], 0, a["rho2"], 0,
                                  a["rho2n"], 0, llh, last, 3, L, L, a["otf"], a["zin"], a["u1o"], a["wo"],
                                  a["saved"], a["ws"], None)


def _bwd(lib, p, llh=POIS, last=0, L=48, **over):
    a = dict(gzin=p[0], gu1o=p[1], gwo=p[2], y=p[3], alpha=p[4], rho1=p[5], rho2=p[6], rho2n=p[7], otf=p[8],
             saved=p[9], gz=p[10], gu1=p[11], gw=p[12], part=p[13], ws=p[14])
    a.update(over)
    return lib.gd_admm_train_iter_backward(a["gzin"], a["gu1o"], a["gwo"], a["y"], a["alpha"], 0, a["rho1"], 0,
                                           a["rho2"], 0, a["rho2n"], 0, llh, last, 3, L, L, a["otf"], a["saved"],
                                           a["gz"], a["gu1"], a["gw"], a["part"], a["ws"], None)


def test_argument_errors_need_no_device(lib):
    keep, p = _bufs(15)
    # bad likelihood
    assert _iter(lib, p, llh=2) == -1
    assert _bwd(lib, p, llh=-1) == -1
    assert b"llh" in lib.gd_last_error()
    # an output that is one of the inputs the graph still holds, or two outputs in one buffer
    assert _iter(lib, p, u1o=p[2]) == -1                 # u1 updated in place
    assert b"alias" in lib.gd_last_error()
    assert _iter(lib, p, wo=p[3]) == -1                  # w updated in place
    assert _iter(lib, p, zin=p[1]) == -1                 # z overwritten (gd_admm_iter allows it, training must not)
    assert _iter(lib, p, zin=p[0]) == -1
    assert _iter(lib, p, u1o=p[9]) == -1                 # u1_out == zin_or_out
    assert _bwd(lib, p, gz=p[0]) == -1                   # g_z over g_zin
    assert _bwd(lib, p, gw=p[2]) == -1
    assert _bwd(lib, p, gu1=p[10]) == -1                 # g_u1 == g_z
    # unsupported side
    assert _iter(lib, p, L=4097) == -2
    assert _bwd(lib, p, L=4097) == -2
    assert lib.gd_admm_train_init(p[0], p[1], 0, 48, 48, p[2], 0, 3, 4097, 4097, p[3], p[4], p[5], p[6], None) == -2
    # required pointers
    assert _iter(lib, p, rho2n=None) == -1               # not last: rho2_next is read
    assert _iter(lib, p, saved=None) == -1
    assert _bwd(lib, p, part=None) == -1
    assert lib.gd_admm_train_init(p[0], p[1], 0, 47, 47, p[2], 0, 3, 48, 48, p[3], p[4], p[5], p[6], None) == -1  # odd PSF
    assert lib.gd_admm_train_init(p[0], p[1], 0, 48, 48, p[2], 0, 3, 48, 48, p[3], p[4], p[4], p[6], None) == -1  # x0 == hx0
    # an empty batch is valid and launches nothing
    assert lib.gd_admm_train_iter(p[0], p[1], p[2], p[3], p[4], 0, p[5], 0, p[6], 0, p[7], 0, POIS, 0, 0, 48, 48,
                                  p[8], p[9], p[10], p[11], p[12], p[13], None) == 0
    del keep


@pytest.mark.parametrize("subnet", [True, False])
def test_trainable_keys_equal_the_inference_class(subnet):
    from gdeconv.models import TrainableUnrolledADMM, Unrolled_ADMM
    a = Unrolled_ADMM(n_iters=3, llh="Poisson", subnet=subnet)
    b = TrainableUnrolledADMM(n_iters=3, llh="Poisson", subnet=subnet)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert isinstance(b, Unrolled_ADMM)
    b.load_state_dict(a.state_dict())          # checkpoints move between the two classes
    a.load_state_dict(b.state_dict())
    for k in ("n", "llh", "PnP", "subnet", "denoiser"):
        assert getattr(a, k) == getattr(b, k)


def test_trainable_is_exported():
    import gdeconv.models as M
    assert "TrainableUnrolledADMM" in M.__all__
    from models.Unrolled_ADMM import TrainableUnrolledADMM
    assert TrainableUnrolledADMM is M.TrainableUnrolledADMM
    assert "inference-only" in M.__doc__ and "TrainableUnrolledADMM" in M.__doc__


@pytest.mark.parametrize("grad", [True, False])
def test_trainable_rejects_cpu_tensors(grad):
    from gdeconv.models import TrainableUnrolledADMM
    m = TrainableUnrolledADMM(n_iters=2, llh="Gaussian", subnet=False)
    m.Z = torch.nn.Identity()
    y, k, al = torch.rand(2, 1, 32, 32), torch.rand(2, 1, 16, 16), torch.ones(2, 1, 1, 1)
    with torch.set_grad_enabled(grad), pytest.raises(ValueError, match="ROCm"):
        m(y, k, al)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_trainable_rejects_inputs_that_require_grad(which):
    from gdeconv.models import TrainableUnrolledADMM
    m = TrainableUnrolledADMM(n_iters=2, llh="Poisson", subnet=False)
    m.Z = torch.nn.Identity()
    ins = [torch.rand(2, 1, 32, 32), torch.rand(2, 1, 16, 16), torch.ones(2, 1, 1, 1)]
    ins[which].requires_grad_()
    with pytest.raises(NotImplementedError, match="requires grad"):
        m(*ins)
