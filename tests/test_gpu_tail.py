"""The combined tail of the 256^2 Gaussian iteration (k_gal_reg): the second-to-last iteration stores
C = rho2' W~' - rho1' U1' in the W~ slot instead of U1' and W~', the last one computes x = (rho1 Z + C) / (rho1 |H|^2
+ rho2) from it.  Checked against the oracle, against the same forward with the tail off (gd_set_combined_tail(0)),
in the state buffer itself (the U1 slot is not written), for misuse, and under a hipGraph replay.

Run on the MI355X box:  python -m pytest tests/test_gpu_tail.py -m gpu -q
"""
import contextlib

import pytest
import torch

import admm_oracle as O
from conftest import TOL

pytestmark = pytest.mark.gpu

L = 256
K = L // 2 + 1


def nerr(out, ref):
    return float(O.normwise_error(out, ref).max())


def denoise(zin):
    """A deterministic Z step that returns a tensor of its own (never the engine's zin buffer)."""
    return 0.9 * zin + 0.05 * torch.roll(zin, 1, -1)


class Denoiser(torch.nn.Module):
    def forward(self, zin):
        return denoise(zin)


@pytest.fixture(scope="module")
def lib():
    from gdeconv import _lib
    return _lib.load()


@contextlib.contextmanager
def fused_min_batch(lib, n):
    old = lib.gd_set_fused_min_batch(0, n)
    try:
        yield
    finally:
        lib.gd_set_fused_min_batch(0, old)


@contextlib.contextmanager
def combined_tail(lib, on):
    old = lib.gd_set_combined_tail(on)
    try:
        yield
    finally:
        lib.gd_set_combined_tail(old)


def case(N, n, dev):
    from gdeconv.synth import make_batch
    obs, psf, alpha, _ = make_batch(N, L, seed=900 + 10 * n + N, device=dev)
    gen = torch.Generator().manual_seed(100 * N + n)
    rho1 = (0.5 + torch.rand(N, 1, 1, n, generator=gen)).to(dev)
    rho2 = (0.5 + torch.rand(N, 1, 1, n, generator=gen)).to(dev)
    return obs, psf, alpha, rho1, rho2


def model(n, dev, rho1, rho2):
    from gdeconv.models import Unrolled_ADMM
    m = Unrolled_ADMM(n_iters=n, llh="Gaussian").to(dev).eval()
    m.Z = Denoiser()
    m.rhos = lambda k, a: (rho1, rho2)
    return m


def on_and_off(lib, m, obs, psf, alpha):
    with torch.no_grad():
        with combined_tail(lib, 1):
            on = m(obs, psf, alpha).cpu()
        with combined_tail(lib, 0):
            off = m(obs, psf, alpha).cpu()
    return on, off


def check_parity(on, off, idx, obs, psf, alpha, rho1, rho2):
    ref = O.admm_forward(obs[idx].cpu(), psf[idx].cpu(), alpha[idx].cpu(), rho1[idx].cpu(), rho2[idx].cpu(),
                         "Gaussian", denoise=denoise)
    e_on, e_off, d = nerr(on[idx], ref), nerr(off[idx], ref), nerr(on, off)
    print(f"[tail] vs oracle: tail on {e_on:.3e}, tail off {e_off:.3e}; on vs off {d:.3e}; "
          f"bitwise equal: {torch.equal(on, off)}")
    assert e_on < TOL and e_off < TOL
    # the bar tests/test_gpu_parity.py sets between two fp32 paths of this iteration.  Bitwise equality is NOT
    # required: C is rounded once where U1' and W~' were rounded separately (torch.equal may be False)
    assert d < 2e-6


@pytest.mark.parametrize("n", [2, 3, 4])
def test_tail_matches_oracle_and_tail_off_small_batch(dev, lib, n):
    """N = 3 through the whole-galaxy kernels; n = 2: the tail-write is the FIRST iteration, n >= 3: a MID one."""
    N = 3
    obs, psf, alpha, rho1, rho2 = case(N, n, dev)
    m = model(n, dev, rho1, rho2)
    with fused_min_batch(lib, 0):
        assert lib.gd_admm_tail_supported(N, L, L, 0) == 1
        on, off = on_and_off(lib, m, obs, psf, alpha)
    check_parity(on, off, [0, 1, 2], obs, psf, alpha, rho1, rho2)


def test_tail_matches_oracle_and_tail_off_default_routing(dev, lib):
    N, n = 97, 3
    assert lib.gd_set_fused_min_batch(0, -1) == 96
    obs, psf, alpha, rho1, rho2 = case(N, n, dev)
    m = model(n, dev, rho1, rho2)
    on, off = on_and_off(lib, m, obs, psf, alpha)
    check_parity(on, off, [0, 96], obs, psf, alpha, rho1, rho2)


def slots(lib, N):
    """Byte ranges (U1 slot, W~ slot) of the 256^2 Gaussian state, from gd_admm_state_bytes' formula
    ([|H|^2 fp32 | G | U1 | W~], 256 KiB between the slots): W~ is the last N K L complex, U1 the slot before."""
    spec, gap = N * K * L * 8, 256 * 1024
    total = (N * K * L + 1) // 2 * 8 + 3 * spec + 3 * gap
    assert lib.gd_admm_state_bytes(N, L, L, 0) == total
    w0 = total - spec
    u0 = w0 - gap - spec
    return (u0, u0 + spec), (w0, total)


def drive(lib, st, rho1, rho2, n, upto, give_rho1_next=True):
    """init + iterations [0, upto) of an n-iteration forward on ``st``; returns the state bytes before and after
    the last of them."""
    from gdeconv import engine
    N = st.N
    r1, r2 = engine.RhoSchedule(rho1, N, st.dev), engine.RhoSchedule(rho2, N, st.dev)
    out = torch.empty_like(st.y)
    st.init(None)
    before = None
    for it in range(upto):
        z = denoise(st.zin)
        if it == upto - 1:
            before = st.state.clone()
        st.step(z, r1[it], r2[it], r2[it + 1] if it + 1 < n else None, out=out,
                rho1_next=r1[it + 1] if (it == n - 2 and give_rho1_next) else None)
    return before, st.state.clone(), (r1, r2, out)


@pytest.mark.parametrize("n", [2, 3])
def test_tail_write_leaves_the_u1_slot_alone(dev, lib, n):
    from gdeconv import engine
    N = 3
    obs, psf, alpha, rho1, rho2 = case(N, n, dev)
    (u0, u1), (w0, w1) = slots(lib, N)
    with fused_min_batch(lib, 0), torch.no_grad():
        with combined_tail(lib, 1):
            st = engine.ADMMState(obs, psf, alpha, "Gaussian")
            before, after, _ = drive(lib, st, rho1, rho2, n, upto=n - 1)
        changed = (before != after)
        assert bool(changed[w0:w1].any())
        assert not bool(changed[:w0].any()), "a byte outside the W~ slot changed"
        assert torch.equal(before[u0:u1], after[u0:u1])
        with combined_tail(lib, 0):
            st = engine.ADMMState(obs, psf, alpha, "Gaussian")
            before, after, _ = drive(lib, st, rho1, rho2, n, upto=n - 1)
        assert not torch.equal(before[u0:u1], after[u0:u1]), "tail off: the iteration stores U1'"
        assert not torch.equal(before[w0:w1], after[w0:w1])


def test_misuse_raises(dev, lib):
    from gdeconv import _lib, engine
    N, n = 3, 4
    obs, psf, alpha, rho1, rho2 = case(N, n, dev)
    with fused_min_batch(lib, 0), combined_tail(lib, 1), torch.no_grad():
        # a non-last step after the tail-write (issued at iteration 1 as if n were 3)
        st = engine.ADMMState(obs, psf, alpha, "Gaussian")
        _, _, (r1, r2, out) = drive(lib, st, rho1, rho2, 3, upto=2)
        with pytest.raises(_lib.EngineError):
            st.step(denoise(st.zin), r1[2], r2[2], r2[3], out=out)
        # the routing toggled between the tail-write and the last step: the chained kernels would read C as W~
        st = engine.ADMMState(obs, psf, alpha, "Gaussian")
        _, _, (r1, r2, out) = drive(lib, st, rho1, rho2, 3, upto=2)
        old = lib.gd_set_fused_iteration(0)
        try:
            with pytest.raises(_lib.EngineError):
                st.step(denoise(st.zin), r1[2], r2[2], None, out=out)
        finally:
            lib.gd_set_fused_iteration(old)
        # with the routing restored the same state still finishes
        st.step(denoise(st.zin), r1[2], r2[2], None, out=out)
        assert torch.isfinite(out).all()


def test_graph_replay_bit_identical(dev, lib):
    from gdeconv.graphs import GraphedForward
    N, n = 3, 3
    obs, psf, alpha, rho1, rho2 = case(N, n, dev)
    m = model(n, dev, rho1, rho2)
    with fused_min_batch(lib, 0), combined_tail(lib, 1):
        with torch.no_grad():
            eager = m(obs, psf, alpha).clone()
        g = GraphedForward(m, obs, psf, alpha, clone=True)
        assert torch.equal(g(obs, psf, alpha), eager)
