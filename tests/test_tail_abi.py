"""The combined-tail entry points of the C ABI (gd_admm_iter_tail, gd_admm_tail_supported, gd_set_combined_tail):
routing query, strict switch and argument validation.  Host only: every call here returns before any HIP call."""
import ctypes
import os

import pytest

from conftest import ROOT

GAUSS, POIS = 0, 1


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


def test_abi_version_unchanged(lib):
    assert lib.gd_abi_version() == 5


def test_tail_supported_follows_the_routing(lib):
    """1 exactly where gd_admm_iter runs k_gal_reg: Gaussian, 256^2, fused iteration on, batch at or above the fused
    minimum, combined tail on."""
    q = lib.gd_admm_tail_supported
    old_t = lib.gd_set_combined_tail(1)
    try:
        assert q(4096, 256, 256, GAUSS) == 1
        assert q(64, 256, 256, GAUSS) == 0       # below gd_set_fused_min_batch: the chained kernels
        assert q(4096, 256, 256, POIS) == 0
        assert q(256, 48, 48, GAUSS) == 0
        old_f = lib.gd_set_fused_iteration(0)
        try:
            assert q(4096, 256, 256, GAUSS) == 0
        finally:
            lib.gd_set_fused_iteration(old_f)
        assert q(4096, 256, 256, GAUSS) == 1
        assert lib.gd_set_combined_tail(0) == 1
        assert q(4096, 256, 256, GAUSS) == 0
    finally:
        lib.gd_set_combined_tail(old_t)


def test_combined_tail_setter_is_strict(lib):
    f = lib.gd_set_combined_tail
    cur = f(1)
    try:
        assert cur in (0, 1)
        assert f(2) == -1 and f(-1) == -1
        assert f(1) == 1                         # still 1 after the refused values
        assert f(0) == 1 and f(3) == -1 and f(0) == 0
    finally:
        f(cur)


def _iter_tail(lib, last, rho1_next, tail, N=4096, L=256):
    # every pointer NULL except (optionally) rho1_next: validation must return before anything is dereferenced
    return lib.gd_admm_iter_tail(None, None, None, None, 0, None, 0, None, 0, None, 0, GAUSS, 1, last, N, L, L,
                                 None, None, None, rho1_next, 0, tail)


def test_tail_argument_errors_need_no_device(lib):
    dummy = ctypes.c_float(1.0)                  # a non-NULL rho1_next (host memory: never read by these calls)
    r1n = ctypes.addressof(dummy)
    old = lib.gd_set_combined_tail(1)
    try:
        assert _iter_tail(lib, last=1, rho1_next=r1n, tail=1) == -1     # a tail-write is never the last call
        assert _iter_tail(lib, last=0, rho1_next=None, tail=1) == -1    # it needs rho1_next
        assert b"rho1_next" in lib.gd_last_error()
        assert _iter_tail(lib, last=0, rho1_next=r1n, tail=2) == -1     # a tail-read is the last call
        assert _iter_tail(lib, last=0, rho1_next=r1n, tail=3) == -1
        assert _iter_tail(lib, last=0, rho1_next=r1n, tail=1, N=256, L=48) == -2   # k_gal_small: no tail
        assert _iter_tail(lib, last=1, rho1_next=None, tail=2, N=256, L=48) == -2
        assert _iter_tail(lib, last=0, rho1_next=r1n, tail=1, N=64) == -2          # 256^2 below the fused minimum
        v = (ctypes.c_longlong * 23)()
        v[11], v[12], v[13], v[14], v[15], v[16], v[22] = GAUSS, 1, 1, 4096, 256, 256, 1
        assert lib.gd_admm_iter_tail_v(ctypes.addressof(v)) == -1       # tail = 1 with last = 1, packed form
        assert lib.gd_admm_iter_tail_v(None) == -1
    finally:
        lib.gd_set_combined_tail(old)
