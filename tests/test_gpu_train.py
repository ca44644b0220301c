"""Training ``Unrolled_ADMM`` on the engine: gd_admm_train_iter / gd_admm_train_iter_backward through
``engine.admm_train_iter`` and ``TrainableUnrolledADMM``.

Reference: ``torch.autograd`` through the oracle on the CPU in fp64.  Gradient metric: max|g - g64| / max|g64| over the
whole tensor; gate err_engine <= max(1e-5, 3 err_ref32), err_ref32 being the same oracle in fp32 on the same inputs
(the factor 3 covers the engine's different reduction order: per-column parts, half-spectrum weights).  Outputs keep the
1e-5 per-galaxy normwise bar."""
import copy

import pytest
import torch
import torch.nn.functional as F

import admm_oracle as O
from gdeconv.synth import make_batch

pytestmark = pytest.mark.gpu
TOL = 1e-5


def gerr(g, g64):
    g, g64 = g.detach().double().cpu().reshape(-1), g64.detach().double().cpu().reshape(-1)
    return float((g - g64).abs().max() / g64.abs().max())


def gate(tag, got, ref32, ref64):
    e, e32 = gerr(got, ref64), gerr(ref32, ref64)
    print(f"[train-grad] {tag}: engine {e:.3e}, oracle fp32 {e32:.3e}, bound {max(TOL, 3 * e32):.3e}")
    assert torch.isfinite(got).all(), tag
    assert e <= max(TOL, 3 * e32), (tag, e, e32)


def out_gate(tag, out, ref64):
    e = float(O.normwise_error(out, ref64).max())
    print(f"[train-out] {tag}: {e:.3e}")
    assert e <= TOL, (tag, e)


def seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)


class Denoiser(torch.nn.Module):
    """A seeded 3x3 conv2d times a learnable scale; returns a new tensor.  ``shifted``: the same convolution as nine
    shifted slices of the zero-padded input times the taps, whose backward is plain elementwise ops and sums (the
    library's convolution weight gradient is not reproducible from run to run, which would hide what the bit-identity
    tests are about: the engine)."""

    def __init__(self, seed=11, shifted=False):
        super().__init__()
        self.shifted = shifted
        g = torch.Generator().manual_seed(seed)
        w = 0.05 * torch.randn(1, 1, 3, 3, generator=g, dtype=torch.float64)
        w[0, 0, 1, 1] += 1.0
        self.weight = torch.nn.Parameter(w.float())
        self.scale = torch.nn.Parameter(torch.tensor(0.9))

    def forward(self, x):
        if self.shifted:
            Hh, Ww = x.shape[-2:]
            xp = F.pad(x, (1, 1, 1, 1))
            out = sum(self.weight[0, 0, i, j] * xp[:, :, i:i + Hh, j:j + Ww] for i in range(3) for j in range(3))
            return out * self.scale
        return F.conv2d(x, self.weight.to(x.dtype), padding=1) * self.scale.to(x.dtype)


# ----------------------------------------------------------------------------- 1. one body against the oracle's ops
def ref_body(y, H, alpha, z, u1, w, r1, r2, r2n, llh, last):
    """The loop body of models/Unrolled_ADMM.py:207-215 on the state (u1, w = v - u2), from the oracle's ops."""
    yp = torch.clamp_min(y, 0)
    Ht, HtH = torch.conj(H), torch.abs(H) ** 2
    x = O.x_update(z - u1, O.conv_fft_batch(Ht, w), HtH, r1, r2)
    if last:
        return (x * alpha if llh == "Poisson" else x,)
    hx = O.conv_fft_batch(H, x)
    u1n = u1 + x - z
    u2 = hx - w
    vt = hx + u2
    v = O.v_update_poisson(vt, yp, r2n, alpha) if llh == "Poisson" else O.v_update_gaussian(vt, yp / alpha, r2n)
    return x + u1n, u1n, v - u2


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
@pytest.mark.parametrize("shape", [(48, 48, 48), (33, 45, 16)])
def test_single_body(dev, shape, llh, last):
    from gdeconv import engine
    Hh, Ww, h = shape
    N = 3
    y, psf, alpha, _ = make_batch(N, Hh, Ww, h=h, seed=31)
    st = engine.ADMMTrainState(y.to(dev), psf.to(dev), alpha.to(dev), llh)
    rho = [(0.5 + seeded((N, 1, 1, 1), 40 + i)) for i in range(3)]
    x0, hx0 = st.x0.cpu().double(), st.hx0.cpu().double()
    # a realistic state: z near x0, small u1, w near the first V step's output
    yp64, al64 = y.double().clamp_min(0), alpha.double()
    w0 = (O.v_update_poisson(hx0, yp64, rho[1], al64) if llh == "Poisson"
          else O.v_update_gaussian(hx0, yp64 / al64, rho[1]))
    g = torch.Generator().manual_seed(7)
    noise = lambda s: s * torch.randn(y.shape, generator=g, dtype=torch.float64)  # noqa: E731
    state64 = [x0 + noise(0.02), noise(0.01), w0 + noise(0.02 * float(w0.abs().max()))]
    nout = 1 if last else 3
    R = [torch.randn(y.shape, generator=g, dtype=torch.float64) for _ in range(nout)]

    def run_ref(dt):
        _, H = O.psf_to_otf(psf.to(dt), y.size(), dtype=dt)
        leaves = [t.to(dt).requires_grad_() for t in state64 + rho]
        outs = ref_body(y.to(dt), H, alpha.to(dt), *leaves, llh, last)
        loss = sum((o * r.to(dt)).sum() for o, r in zip(outs, R))
        grads = torch.autograd.grad(loss, leaves[:5] if last else leaves)
        return outs, grads

    o64, g64 = run_ref(torch.float64)
    o32, g32 = run_ref(torch.float32)
    leaves = [t.float().to(dev).requires_grad_() for t in state64 + rho]
    outs = engine.admm_train_iter(st, *leaves, bool(last))
    outs = (outs,) if last else outs
    loss = sum((o * r.float().to(dev)).sum() for o, r in zip(outs, R))
    grads = torch.autograd.grad(loss, leaves[:5] if last else leaves)
    tag = f"body {Hh}x{Ww} {llh} last={last}"
    for name, o, r in zip(("zin|out", "u1", "w"), outs, o64):
        out_gate(f"{tag} {name}", o, r)
    for name, a, b, c in zip(("g_z", "g_u1", "g_w", "g_rho1", "g_rho2", "g_rho2n"), grads, g32, g64):
        gate(f"{tag} {name}", a, b, c)


# ----------------------------------------------------------------------------- 2. the whole loop
LOOP_CASES = [  # (H, W, PSF side, N, n, rho schedule)
    (48, 48, 48, 3, 3, "per_galaxy"),
    (32, 32, 16, 3, 2, "per_galaxy"),
    (40, 56, 24, 3, 3, "per_galaxy"),
    (48, 48, 48, 1, 4, "shared"),
    (48, 48, 48, 7, 2, "shared"),
    (256, 256, 48, 2, 2, "per_galaxy"),
]


def loop_inputs(case, seed=20250307):
    Hh, Ww, h, N, n, sched = case
    y, psf, alpha, _ = make_batch(N, Hh, Ww, h=h, seed=seed)
    shp = (N, 1, 1, n) if sched == "per_galaxy" else (n,)
    rho1, rho2 = 0.5 + seeded(shp, 101), 0.5 + seeded(shp, 102)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(103), dtype=torch.float64)
    return y, psf, alpha, rho1, rho2, R


def loop_reference(case, llh, dt):
    """(out, {name: grad}) of autograd through oracle.admm_forward on the CPU in dtype ``dt``."""
    y, psf, alpha, rho1, rho2, R = loop_inputs(case)
    den = Denoiser().to(dt)
    r1, r2 = rho1.to(dt).requires_grad_(), rho2.to(dt).requires_grad_()
    out = O.admm_forward(y.to(dt), psf.to(dt), alpha.to(dt), r1, r2, llh, denoise=den)
    (out * R.to(dt)).sum().backward()
    return out.detach(), {"rho1": r1.grad, "rho2": r2.grad, "weight": den.weight.grad, "scale": den.scale.grad}


def loop_engine(case, llh, dev, shifted=False):
    """(out, {name: grad}) of TrainableUnrolledADMM with the same denoiser and schedule."""
    from gdeconv.models import TrainableUnrolledADMM
    Hh, Ww, h, N, n, sched = case
    y, psf, alpha, rho1, rho2, R = loop_inputs(case)
    m = TrainableUnrolledADMM(n_iters=n, llh=llh, subnet=False)
    m.Z = Denoiser(shifted=shifted)
    m = m.to(dev).train()
    if sched == "shared":
        with torch.no_grad():
            m.rho1_iters.copy_(rho1.float())
            m.rho2_iters.copy_(rho2.float())
        r1, r2 = m.rho1_iters, m.rho2_iters
    else:
        r1, r2 = rho1.float().to(dev).requires_grad_(), rho2.float().to(dev).requires_grad_()
        m.rhos = lambda k, a: (r1, r2)
    out = m(y.to(dev), psf.to(dev), alpha.to(dev))
    assert out.requires_grad
    (out * R.float().to(dev)).sum().backward()
    return out.detach(), {"rho1": r1.grad.clone(), "rho2": r2.grad.clone(), "weight": m.Z.weight.grad.clone(),
                          "scale": m.Z.scale.grad.clone()}


_REF = {}


def loop_refs(case, llh):
    key = (case, llh)
    if key not in _REF:
        _REF[key] = (loop_reference(case, llh, torch.float64), loop_reference(case, llh, torch.float32))
    return _REF[key]


@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
@pytest.mark.parametrize("case", LOOP_CASES, ids=lambda c: f"{c[0]}x{c[1]}-psf{c[2]}-N{c[3]}-n{c[4]}-{c[5]}")
def test_whole_loop(dev, case, llh):
    (o64, g64), (o32, g32) = loop_refs(case, llh)
    out, grads = loop_engine(case, llh, dev)
    tag = f"loop {case} {llh}"
    out_gate(tag, out, o64)
    for k in ("rho1", "rho2", "weight", "scale"):
        assert grads[k].shape == g64[k].shape, k
        gate(f"{tag} d/d{k}", grads[k], g32[k], g64[k])


# ----------------------------------------------------------------------------- 3. the full model
@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_full_model(dev, llh):
    """SubNet + ResUNet + the HIP body and adjoint against the same modules on the CPU (fp32) driving the oracle:
    output at 1e-5, parameter gradients at 1e-4.

    The input seed is chosen by the reference's own conditioning, not by the engine: with ReLU networks the loss is
    piecewise smooth, and where a high-leverage pre-activation sits within fp32 rounding of zero the reference's own
    gradients in fp32 and fp64 differ by 1e-4 .. 6e-4 on these four tensors (CPU only, input seeds 5 .. 27 with these
    weights: 40 % of the (seed, likelihood) pairs; e.g. seed 5, Poisson: 2.8e-4, and on the GPU three runs of one
    model landed on the fp32 answer twice and on the fp64 answer once, each time within 4e-6 of it).  Seed 16 is the
    one where the CPU reference agrees with itself in fp64 best (<= 1.5e-6 on all four tensors, both likelihoods), so
    the 1e-4 bar measures the engine and the GPU convolutions, not which side of a kink a rounding error fell."""
    from gdeconv.models import TrainableUnrolledADMM
    from gdeconv.weights import make_state_dict
    m = TrainableUnrolledADMM(n_iters=2, llh=llh)
    m.load_state_dict(make_state_dict(m, 1234))
    m = m.eval()
    Z_cpu, init_cpu = copy.deepcopy(m.Z), copy.deepcopy(m.init)
    m = m.to(dev)
    y, psf, alpha, _ = make_batch(2, 48, h=48, seed=16)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
    out = m(y.to(dev), psf.to(dev), alpha.to(dev))
    assert out.requires_grad
    (out * R.to(dev)).sum().backward()
    rho1, rho2 = init_cpu(psf, alpha)
    ref = O.admm_forward(y, psf, alpha, rho1, rho2, llh, denoise=Z_cpu)
    (ref * R).sum().backward()
    out_gate(f"full model {llh}", out, ref)
    got, want = dict(m.named_parameters()), {**{"Z." + k: v for k, v in Z_cpu.named_parameters()},
                                             **{"init." + k: v for k, v in init_cpu.named_parameters()}}
    for k in ("init.mlp.4.weight", "init.mlp.4.bias", "Z.net.m_tail.weight", "Z.net.m_head.weight"):
        e = gerr(got[k].grad, want[k].grad)
        print(f"[train-grad] full model {llh} {k}: {e:.3e}")
        assert torch.isfinite(got[k].grad).all(), k
        assert e < 1e-4, (k, e)


# ----------------------------------------------------------------------------- 4. chunking and determinism
@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_chunked_and_repeated_runs_are_bit_identical(dev, llh):
    from gdeconv import _lib
    lib = _lib.load()
    case = (64, 64, 48, 7, 2, "per_galaxy")
    per_galaxy_ws = 2 * 33 * 64 * 8
    old_b = lib.gd_set_chunk_bytes(0)
    old_s = lib.gd_set_pipeline_streams(3)
    try:
        one, g_one = loop_engine(case, llh, dev, True)                      # one pass over the batch
        again, g_again = loop_engine(case, llh, dev, True)
        lib.gd_set_chunk_bytes(3 * per_galaxy_ws)                     # chunks of 3, 3, 1 galaxies
        chunked, g_chunked = loop_engine(case, llh, dev, True)
    finally:
        lib.gd_set_chunk_bytes(old_b)
        lib.gd_set_pipeline_streams(old_s)
    assert torch.isfinite(one).all()
    assert torch.equal(one, again) and torch.equal(one, chunked)
    for k in g_one:
        assert torch.equal(g_one[k], g_again[k]), k
        assert torch.equal(g_one[k], g_chunked[k]), k


# ----------------------------------------------------------------------------- 5. routing independence
@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_routing_switches_do_not_reach_training(dev, llh):
    from gdeconv import _lib
    lib = _lib.load()
    old = lib.gd_set_fused_iteration(1)
    try:
        on, g_on = loop_engine(LOOP_CASES[0], llh, dev, True)
        lib.gd_set_fused_iteration(0)
        off, g_off = loop_engine(LOOP_CASES[0], llh, dev, True)
    finally:
        lib.gd_set_fused_iteration(old)
    assert torch.equal(on, off)
    for k in g_on:
        assert torch.equal(g_on[k], g_off[k]), k


# ----------------------------------------------------------------------------- 6. the fast path is the parent's
@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_no_grad_is_the_inference_path(dev, llh):
    from gdeconv.models import TrainableUnrolledADMM, Unrolled_ADMM
    from gdeconv.weights import make_state_dict
    a = Unrolled_ADMM(n_iters=3, llh=llh)
    a.load_state_dict(make_state_dict(a, 77))
    b = TrainableUnrolledADMM(n_iters=3, llh=llh)
    b.load_state_dict(a.state_dict())
    a.Z, b.Z = torch.nn.Identity(), torch.nn.Identity()
    a, b = a.to(dev).eval(), b.to(dev).eval()
    y, psf, alpha, _ = make_batch(3, 48, h=48, seed=9)
    y, psf, alpha = y.to(dev), psf.to(dev), alpha.to(dev)
    with torch.no_grad():
        oa, ob = a(y, psf, alpha), b(y, psf, alpha)
    assert not ob.requires_grad
    assert torch.equal(oa, ob)
    for p in b.parameters():
        p.requires_grad_(False)
    assert torch.equal(oa, b(y, psf, alpha))         # grad mode on, nothing to differentiate: still the fast path


@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_train_mode_output_carries_the_graph(dev, llh):
    from gdeconv.models import TrainableUnrolledADMM
    m = TrainableUnrolledADMM(n_iters=3, llh=llh, subnet=False)
    m.Z = torch.nn.Identity()
    m = m.to(dev).train()
    y, psf, alpha, _ = make_batch(2, 48, h=48, seed=9)
    out = m(y.to(dev), psf.to(dev), alpha.to(dev))
    assert out.requires_grad
    out.square().mean().backward()
    for p in (m.rho1_iters, m.rho2_iters):
        assert p.grad is not None and p.grad.shape == (3,)
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0


def test_zero_iterations_returns_the_init(dev):
    from gdeconv.models import TrainableUnrolledADMM, Unrolled_ADMM
    y, psf, alpha, _ = make_batch(2, 48, h=48, seed=9)
    y, psf, alpha = y.to(dev), psf.to(dev), alpha.to(dev)
    for llh in ("Poisson", "Gaussian"):
        t = TrainableUnrolledADMM(n_iters=0, llh=llh, subnet=False).to(dev).train()
        t.extra = torch.nn.Parameter(torch.zeros(1, device=dev))   # something that requires grad: the training path
        with torch.no_grad():
            want = Unrolled_ADMM(n_iters=0, llh=llh, subnet=False).to(dev).eval()(y, psf, alpha)
        got = t(y, psf, alpha)
        assert float(O.normwise_error(got, want).max()) <= TOL
