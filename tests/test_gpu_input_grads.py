"""Input gradients of ``Unrolled_ADMM`` on the engine: d/dy, d/dPSF, d/dalpha through gd_psf_to_otf_backward,
gd_conv_fft_batch_backward_otf, gd_admm_train_iter_full / _full_backward and ``DifferentiableUnrolledADMM``.

Reference: ``torch.autograd`` through the oracle on the CPU in fp64 (the oracle is differentiable in y, kernel and
alpha).  Gradient metric: max|g - g64| / max|g64| over the whole tensor; gate err_engine <= max(1e-5, 3 err_ref32),
err_ref32 being the same oracle in fp32 on the same inputs.  Outputs keep the 1e-5 per-galaxy normwise bar.

Input gradients pass through clamp(x0raw, 0, 1); a pixel within fp32 rounding of a kink flips the mask on one side only.
Every oracle-compared case that differentiates the init therefore first asserts, from the fp64 oracle, that no x0raw
pixel lies within 1e-5 max|x0raw| of 0 or of 1 (``assert_no_kink``); the seeds are chosen to meet it."""
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


def gate(tag, got, ref32, ref64, floor=TOL):
    """err_engine <= max(floor, 3 err_ref32).  A gradient the reference does not have (None: the input is unused, e.g.
    y in a last body) must be None or exactly zero on the engine."""
    if ref64 is None or float(ref64.abs().max()) == 0.0:
        assert got is None or float(got.abs().max()) == 0.0, tag
        print(f"[input-grad] {tag}: no gradient on either side")
        return
    assert got is not None, tag
    assert tuple(got.shape) == tuple(ref64.shape), (tag, got.shape, ref64.shape)
    e, e32 = gerr(got, ref64), gerr(ref32, ref64)
    print(f"[input-grad] {tag}: engine {e:.3e}, oracle fp32 {e32:.3e}, bound {max(floor, 3 * e32):.3e}")
    assert torch.isfinite(got).all(), tag
    assert e <= max(floor, 3 * e32), (tag, e, e32)


def out_gate(tag, out, ref64):
    e = float(O.normwise_error(out, ref64).max())
    print(f"[input-out] {tag}: {e:.3e}")
    assert e <= TOL, (tag, e)


def seeded(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)


def x0raw64(y, psf, alpha):
    """init_l2 before its clamp (models/Unrolled_ADMM.py:170-175), fp64, from the oracle's ops."""
    y = y.double().clamp_min(0)
    alpha = alpha.double()
    _, H = O.psf_to_otf(psf.double(), y.size(), dtype=torch.float64)
    Ht, HtH = torch.conj(H), torch.abs(H) ** 2
    rhs = O.fftn(O.conv_fft_batch(Ht, y / alpha))
    return O.ifftn(rhs / (HtH + 1 / alpha)).real


def assert_no_kink(y, psf, alpha):
    x = x0raw64(y, psf, alpha)
    m = float(x.abs().max())
    d = float(torch.minimum(x.abs(), (x - 1).abs()).min())
    assert d > 1e-5 * m, f"an x0raw pixel sits {d:.3e} from a clamp kink (max|x0raw| {m:.3e}): pick another seed"
    assert bool((y != 0).all()), "y == 0 exactly: max(y, 0) is not differentiable there"


class Denoiser(torch.nn.Module):
    """A seeded 3x3 conv2d times a learnable scale (tests/test_gpu_train.py's); ``shifted``: the same convolution as
    nine shifted slices, whose backward is reproducible from run to run (the bit-identity tests)."""

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


SHAPES = [(32, 32, 16, 3), (48, 48, 48, 3), (33, 45, 16, 3), (256, 256, 48, 2)]  # (H, W, PSF side, N)
shape_id = lambda s: f"{s[0]}x{s[1]}-psf{s[2]}-N{s[3]}"  # noqa: E731


def half(Hfull, W):
    """[N,1,H,W] full spectrum -> the engine's stored half spectrum [N, W//2+1, H]."""
    return Hfull[:, 0, :, :W // 2 + 1].transpose(1, 2)


def crand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(shape, generator=g, dtype=torch.float64),
                         torch.randn(shape, generator=g, dtype=torch.float64))


# ----------------------------------------------------------------------------- 1. the adjoint of psf_to_otf
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_psf_to_otf_adjoint(dev, shape):
    from gdeconv import engine
    Hh, Ww, h, N = shape
    K = Ww // 2 + 1
    _, psf, _, _ = make_batch(N, Hh, Ww, h=h, seed=31)
    G = crand((N, K, Hh), 5)
    # <psf_to_otf(p), G> = <p, backward(G)> under dL = sum over the stored bins of Re(conj(G) dOTF), relative to |lhs|
    p = seeded(psf.shape, 6, -1.0, 1.0).float().to(dev).requires_grad_()
    otf = engine.psf_to_otf_half(p, N, Hh, Ww)
    assert otf.requires_grad and tuple(otf.shape) == (N, K, Hh)
    (gp,) = torch.autograd.grad(otf, p, grad_outputs=G.to(torch.complex64).to(dev))
    lhs = float((G.conj() * otf.detach().cpu().to(torch.complex128)).real.sum())
    rhs = float((p.detach().cpu().double() * gp.cpu().double()).sum())
    print(f"[input-grad] psf_to_otf dot {shape}: lhs {lhs:.9e} rhs {rhs:.9e} rel {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)

    # dL/dpsf against fp64 autograd through the oracle's psf_to_otf restricted to the half spectrum
    def ref(dt):
        q = psf.detach().to(dt).clone().requires_grad_()
        _, Hf = O.psf_to_otf(q, (N, 1, Hh, Ww), dtype=dt)
        cdt = torch.complex128 if dt == torch.float64 else torch.complex64
        (G.to(cdt).conj() * half(Hf, Ww)).real.sum().backward()
        return q.grad
    q = psf.to(dev).requires_grad_()
    (G.to(torch.complex64).to(dev).conj() * engine.psf_to_otf_half(q, N, Hh, Ww)).real.sum().backward()
    gate(f"psf_to_otf {shape} d/dpsf", q.grad, ref(torch.float32), ref(torch.float64))


def test_psf_to_otf_shared_psf_and_no_graph(dev):
    from gdeconv import engine
    _, psf, _, _ = make_batch(3, 48, 48, h=16, seed=31)
    one = psf[:1].to(dev)
    plain = engine.psf_to_otf_half(one, 3, 48, 48)
    assert not plain.requires_grad                       # nothing requires grad: the plain call, no graph
    q = one.clone().requires_grad_()
    otf = engine.psf_to_otf_half(q, 3, 48, 48)
    assert torch.equal(otf.detach(), plain)
    G = crand((3, 25, 48), 8).to(torch.complex64).to(dev)
    (G.conj() * otf).real.sum().backward()
    assert tuple(q.grad.shape) == (1, 1, 16, 16)         # the gradient takes the input's shape: summed over the batch
    each = psf[:1].expand(3, -1, -1, -1).contiguous().to(dev).requires_grad_()
    (G.conj() * engine.psf_to_otf_half(each, 3, 48, 48)).real.sum().backward()
    assert gerr(q.grad, each.grad.sum(0, keepdim=True)) <= 1e-6


# ----------------------------------------------------------------------------- 2. conv_half
@pytest.mark.parametrize("conj", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_conv_half_gradients(dev, shape, conj):
    from gdeconv import engine
    Hh, Ww, h, N = shape
    y, psf, _, _ = make_batch(N, Hh, Ww, h=h, seed=31)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)

    def ref(dt):
        x, q = y.detach().to(dt).clone().requires_grad_(), psf.detach().to(dt).clone().requires_grad_()
        _, Hf = O.psf_to_otf(q, y.size(), dtype=dt)
        out = O.conv_fft_batch(torch.conj(Hf) if conj else Hf, x)
        (out * R.to(dt)).sum().backward()
        return out.detach(), x.grad, q.grad
    o64, gx64, gp64 = ref(torch.float64)
    _, gx32, gp32 = ref(torch.float32)
    x, q = y.to(dev).requires_grad_(), psf.to(dev).requires_grad_()
    out = engine.conv_half(engine.psf_to_otf_half(q, N, Hh, Ww), x, conj=bool(conj))
    (out * R.float().to(dev)).sum().backward()
    tag = f"conv_half {shape} conj={conj}"
    out_gate(tag, out, o64)
    gate(f"{tag} d/dx", x.grad, gx32, gx64)
    gate(f"{tag} d/dpsf", q.grad, gp32, gp64)
    with torch.no_grad():
        assert torch.equal(engine.conv_half(engine.psf_to_otf_half(q, N, Hh, Ww), x, conj=bool(conj)), out.detach())


# ----------------------------------------------------------------------------- 3. one body, every input
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
    assert bool((y != 0).all())
    ins = [t.to(dev).requires_grad_() for t in (y, psf, alpha)]
    st = engine.ADMMTrainState(*ins, llh, input_grads=True)
    rho = [(0.5 + seeded((N, 1, 1, 1), 40 + i)) for i in range(3)]
    x0, hx0 = st.x0.detach().cpu().double(), st.hx0.detach().cpu().double()
    yp64, al64 = y.double().clamp_min(0), alpha.double()
    w0 = (O.v_update_poisson(hx0, yp64, rho[1], al64) if llh == "Poisson"
          else O.v_update_gaussian(hx0, yp64 / al64, rho[1]))
    g = torch.Generator().manual_seed(7)
    noise = lambda s: s * torch.randn(y.shape, generator=g, dtype=torch.float64)  # noqa: E731
    state64 = [x0 + noise(0.02), noise(0.01), w0 + noise(0.02 * float(w0.abs().max()))]
    nout = 1 if last else 3
    R = [torch.randn(y.shape, generator=g, dtype=torch.float64) for _ in range(nout)]
    names = ["g_y", "g_psf", "g_alpha", "g_z", "g_u1", "g_w", "g_rho1", "g_rho2", "g_rho2n"]

    def run_ref(dt):
        yl, pl, al = (t.detach().to(dt).clone().requires_grad_() for t in (y, psf, alpha))
        _, H = O.psf_to_otf(pl, y.size(), dtype=dt)
        leaves = [t.detach().to(dt).clone().requires_grad_() for t in state64 + rho]
        outs = ref_body(yl, H, al, *leaves, llh, last)
        loss = sum((o * r.to(dt)).sum() for o, r in zip(outs, R))
        return outs, torch.autograd.grad(loss, [yl, pl, al] + leaves, allow_unused=True)

    o64, g64 = run_ref(torch.float64)
    _, g32 = run_ref(torch.float32)
    leaves = [t.float().to(dev).requires_grad_() for t in state64 + rho]
    outs = engine.admm_train_iter(st, *leaves, bool(last))
    outs = (outs,) if last else outs
    loss = sum((o * r.float().to(dev)).sum() for o, r in zip(outs, R))
    grads = torch.autograd.grad(loss, ins + leaves, allow_unused=True)
    tag = f"body {Hh}x{Ww} {llh} last={last}"
    # the _full call's forward outputs are gd_admm_train_iter's to 1e-6 normwise, not bit for bit: the column and
    # row-inverse kernels are separate template instantiations (they differ in what they save), and the compiler
    # contracts the X update's multiply-adds differently in the two, which moves the last bit of a few pixels
    with torch.no_grad():
        plain = engine._ADMMTrainIterFn.apply(*[t.detach() for t in leaves[:5]], None if last else leaves[5].detach(),
                                              st, bool(last))
    for name, a, b in zip(("zin|out", "u1", "w"), outs, (plain,) if last else plain):
        e = float(O.normwise_error(a, b).max())
        print(f"[input-out] {tag} {name}: _full vs gd_admm_train_iter {e:.3e} (equal: {torch.equal(a.detach(), b)})")
        assert e <= 1e-6, (name, e)
    for name, o, r in zip(("zin|out", "u1", "w"), outs, o64):
        out_gate(f"{tag} {name}", o, r)
    for name, a, b, c in zip(names, grads, g32, g64):
        gate(f"{tag} {name}", a, b, c)


# ----------------------------------------------------------------------------- 4. the whole loop
LOOP_CASES = [  # (H, W, PSF side, N, n, rho schedule; "shared": shared rho, one [1,1,h,w] PSF and a scalar alpha)
    (48, 48, 48, 3, 3, "per_galaxy"),
    (32, 32, 16, 3, 2, "per_galaxy"),
    (40, 56, 24, 3, 3, "per_galaxy"),
    (48, 48, 48, 3, 2, "shared"),
    (256, 256, 48, 2, 2, "per_galaxy"),
]
case_id = lambda c: f"{c[0]}x{c[1]}-psf{c[2]}-N{c[3]}-n{c[4]}-{c[5]}"  # noqa: E731
SHARED_SEED = 16   # 20250307 and 31 put an x0raw pixel within 1e-5 max|x0raw| of 1 with the shared PSF and alpha


def loop_inputs(case, seed=20250307):
    Hh, Ww, h, N, n, sched = case
    if sched == "shared":
        y, psf, alpha, _ = make_batch(N, Hh, Ww, h=h, seed=SHARED_SEED)
        psf, alpha = psf[:1].clone(), alpha.mean().reshape(())
    else:
        y, psf, alpha, _ = make_batch(N, Hh, Ww, h=h, seed=seed)
    shp = (N, 1, 1, n) if sched == "per_galaxy" else (n,)
    rho1, rho2 = 0.5 + seeded(shp, 101), 0.5 + seeded(shp, 102)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(103), dtype=torch.float64)
    return y, psf, alpha, rho1, rho2, R


def loop_reference(case, llh, dt):
    """(out, {name: grad}) of autograd through oracle.admm_forward on the CPU in dtype ``dt``."""
    y, psf, alpha, rho1, rho2, R = loop_inputs(case)
    den = Denoiser().to(dt)
    yl, pl, al = (t.detach().to(dt).clone().requires_grad_() for t in (y, psf, alpha))
    r1, r2 = rho1.detach().to(dt).clone().requires_grad_(), rho2.detach().to(dt).clone().requires_grad_()
    out = O.admm_forward(yl, pl, al, r1, r2, llh, denoise=den)
    (out * R.to(dt)).sum().backward()
    return out.detach(), {"y": yl.grad, "kernel": pl.grad, "alpha": al.grad, "rho1": r1.grad, "rho2": r2.grad,
                          "weight": den.weight.grad, "scale": den.scale.grad}


def loop_engine(case, llh, dev, shifted=False, wrt=("y", "kernel", "alpha"), cls=None):
    """(out, {name: grad}) of DifferentiableUnrolledADMM with the same denoiser and schedule; the inputs named in
    ``wrt`` require grad."""
    from gdeconv.models import DifferentiableUnrolledADMM
    Hh, Ww, h, N, n, sched = case
    y, psf, alpha, rho1, rho2, R = loop_inputs(case)
    m = (cls or DifferentiableUnrolledADMM)(n_iters=n, llh=llh, subnet=False)
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
    ins = {"y": y.to(dev), "kernel": psf.to(dev), "alpha": alpha.to(dev)}
    for k in wrt:
        ins[k].requires_grad_()
    out = m(ins["y"], ins["kernel"], ins["alpha"])
    assert out.requires_grad
    (out * R.float().to(dev)).sum().backward()
    grads = {k: (None if v.grad is None else v.grad.clone()) for k, v in ins.items()}
    grads.update({"rho1": r1.grad.clone(), "rho2": r2.grad.clone(), "weight": m.Z.weight.grad.clone(),
                  "scale": m.Z.scale.grad.clone()})
    return out.detach(), grads


_REF = {}


def loop_refs(case, llh):
    key = (case, llh)
    if key not in _REF:
        y, psf, alpha = loop_inputs(case)[:3]
        assert_no_kink(y, psf, alpha)
        _REF[key] = (loop_reference(case, llh, torch.float64), loop_reference(case, llh, torch.float32))
    return _REF[key]


@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
@pytest.mark.parametrize("case", LOOP_CASES, ids=case_id)
def test_whole_loop(dev, case, llh):
    (o64, g64), (o32, g32) = loop_refs(case, llh)
    out, grads = loop_engine(case, llh, dev)
    tag = f"loop {case} {llh}"
    out_gate(tag, out, o64)
    for k in ("y", "kernel", "alpha", "rho1", "rho2", "weight", "scale"):
        gate(f"{tag} d/d{k}", grads[k], g32[k], g64[k])


@pytest.mark.parametrize("only", ["kernel", "y"])
def test_only_one_input_requires_grad(dev, only):
    case, llh = LOOP_CASES[1], "Poisson"
    (o64, g64), (o32, g32) = loop_refs(case, llh)
    out, grads = loop_engine(case, llh, dev, wrt=(only,))
    out_gate(f"loop {case} {llh} only {only}", out, o64)
    for k in ("y", "kernel", "alpha"):
        if k == only:
            gate(f"only {only} d/d{k}", grads[k], g32[k], g64[k])
        else:
            assert grads[k] is None, k
    for k in ("rho1", "rho2", "weight", "scale"):
        gate(f"only {only} d/d{k}", grads[k], g32[k], g64[k])


# ----------------------------------------------------------------------------- 5. the full model
FULL_SEED = 16


def subnet_ref(init, kernel, alpha):
    """``SubNet.forward``'s PyTorch path (models/Unrolled_ADMM.py:77-90) in the dtype of its arguments: the module
    itself casts |FFT2(pad128(psf))|^2 to fp32, which an fp64 reference must not."""
    N, _, h, w = kernel.shape
    h1, h2 = (128 - h) // 2, 128 - h - (128 - h) // 2
    w1, w2 = (128 - w) // 2, 128 - w - (128 - w) // 2
    Hk = torch.fft.fftn(F.pad(kernel, (w1, w2, h1, h2), "constant", 0), dim=[2, 3])
    feat = init.conv_layers(torch.abs(Hk) ** 2)
    feat = torch.cat((feat.view(N, 1, 16 * 8 * 8), alpha.view(N, 1, 1)), dim=2)
    out = init.mlp(feat) + 1e-6
    return out[:, :, 0:init.n].view(N, 1, 1, init.n), out[:, :, init.n:2 * init.n].view(N, 1, 1, init.n)


def full_reference(llh, dt, Z_cpu, init_cpu, seed):
    y, psf, alpha, _ = make_batch(2, 48, h=48, seed=seed)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
    Z, init = copy.deepcopy(Z_cpu).to(dt), copy.deepcopy(init_cpu).to(dt)
    yl, pl, al = (t.detach().to(dt).clone().requires_grad_() for t in (y, psf, alpha))
    rho1, rho2 = subnet_ref(init, pl, al)
    ref = O.admm_forward(yl, pl, al, rho1, rho2, llh, denoise=Z.net)   # the ResUNet itself: Z casts its input to fp32
    (ref * R.to(dt)).sum().backward()
    return ref.detach(), {"y": yl.grad, "kernel": pl.grad, "alpha": al.grad}


@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_full_model(dev, llh):
    """SubNet (PyTorch path, eval mode) + ResUNet + the HIP body and adjoints: gradients to y, kernel and alpha, the
    path through the SubNet's rhos included, against the same modules on the CPU driving the oracle in fp64; bar
    max(1e-4, 3 err_ref32), the 1e-4 being the existing full-model bar.

    The input seed (16, tests/test_gpu_train.py::test_full_model's) is chosen by the reference, not by the engine: it
    meets the clamp-kink condition and, on the CPU this was written on, the fp32 reference agrees with itself in fp64
    on the input gradients (y, kernel, alpha) to 1.05e-6, 9.34e-7, 1.08e-6 (Poisson) and 8.22e-7, 9.63e-7, 1.01e-6
    (Gaussian); seed 20250307 <= 1.5e-6 as well, seed 31 fails the kink condition, seed 9 disagrees by up to 1.7e-3.

    KNOWN TO MISS ITS BAR FOR llh='Gaussian' (measured on the MI355X, six runs, the same every time): engine vs fp64
    4.98e-4 (y), 3.91e-4 (kernel), 4.8e-5 (alpha) against a bound of 1e-4; Poisson passes at 8.1e-7 .. 1.1e-6 on all
    three.  The miss is where the ResUNet's ReLUs switch, not the engine's adjoints:
      * with the ResUNet's ReLUs replaced by SiLU in the model and in the reference alike, everything else the same
        (``test_full_model_smooth_denoiser`` below), the engine is within 1.4e-6 of fp64 on y, kernel and alpha for
        both likelihoods at seeds 16, 5, 11 and 20250307;
      * each piece alone is exact with this test's own batch, alpha and SubNet rhos: one body 6e-7 on all nine
        gradients (both likelihoods, last 0 / 1), the init (x0, hx0) 8e-7;
      * with ReLU the input gradients have two answers 1e-4 .. 1e-3 apart, depending on which side of zero one
        pre-activation falls in fp32, and the CPU reference in fp32 takes either one depending on the host (seed 16
        Poisson: 1.05e-6 on one CPU, 5.28e-5 on another; seed 11: 6.4e-5 / 1.8e-4 and 1.1e-6 / 1.2e-6); where the
        engine's error is large it equals the fp32 reference's own to three digits (seed 5 Poisson: both 6.19e-4 /
        3.13e-4; seed 20250307 Gaussian: both 1.24e-4 / 7.0e-5); perturbing the reference's inputs by 2e-7 relative
        switches it at every one of 47 seeds that meet the clamp condition (about 3e6 ReLU units per forward, so
        about one of them lies within fp32 rounding of zero).
    No seed was found at which the fp32 reference agrees with fp64 on two hosts, so the seed stays the one the
    criterion above selects, and the bar stays as set."""
    from gdeconv.models import DifferentiableUnrolledADMM
    from gdeconv.weights import make_state_dict
    m = DifferentiableUnrolledADMM(n_iters=2, llh=llh)
    m.load_state_dict(make_state_dict(m, 1234))
    m = m.eval()
    Z_cpu, init_cpu = copy.deepcopy(m.Z), copy.deepcopy(m.init)
    m = m.to(dev)
    y, psf, alpha, _ = make_batch(2, 48, h=48, seed=FULL_SEED)
    assert_no_kink(y, psf, alpha)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
    ins = [t.to(dev).requires_grad_() for t in (y, psf, alpha)]
    out = m(*ins)
    assert out.requires_grad
    (out * R.to(dev)).sum().backward()
    o64, g64 = full_reference(llh, torch.float64, Z_cpu, init_cpu, FULL_SEED)
    _, g32 = full_reference(llh, torch.float32, Z_cpu, init_cpu, FULL_SEED)
    out_gate(f"full model {llh}", out, o64)
    for k, t in zip(("y", "kernel", "alpha"), ins):
        gate(f"full model {llh} d/d{k}", t.grad, g32[k], g64[k], floor=1e-4)
    for k in ("init.mlp.4.weight", "Z.net.m_tail.weight"):       # the parameters still get theirs
        assert dict(m.named_parameters())[k].grad is not None, k


def _smooth(mod):
    """Replace every nn.ReLU below ``mod`` by nn.SiLU (same shapes, no parameters)."""
    for name, ch in mod.named_children():
        if isinstance(ch, torch.nn.ReLU):
            setattr(mod, name, torch.nn.SiLU())
        else:
            _smooth(ch)


@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_full_model_smooth_denoiser(dev, llh):
    """``test_full_model`` with the ResUNet's ReLUs replaced by SiLU, in the engine's model and in the fp64 / fp32
    references alike: the same SubNet (PyTorch path, its ReLUs and max-pools kept), weights, shapes and seed, the same
    HIP bodies and adjoints, but a denoiser without kinks, so the comparison with fp64 is as well defined as for the
    whole loop above and takes its bar, max(1e-5, 3 err_ref32) (measured: engine <= 1.4e-6, fp32 reference <= 5.2e-6)."""
    from gdeconv.models import DifferentiableUnrolledADMM
    from gdeconv.weights import make_state_dict
    m = DifferentiableUnrolledADMM(n_iters=2, llh=llh)
    m.load_state_dict(make_state_dict(m, 1234))
    m = m.eval()
    _smooth(m.Z)
    Z_cpu, init_cpu = copy.deepcopy(m.Z), copy.deepcopy(m.init)
    m = m.to(dev)
    y, psf, alpha, _ = make_batch(2, 48, h=48, seed=FULL_SEED)
    assert_no_kink(y, psf, alpha)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
    ins = [t.to(dev).requires_grad_() for t in (y, psf, alpha)]
    out = m(*ins)
    (out * R.to(dev)).sum().backward()
    o64, g64 = full_reference(llh, torch.float64, Z_cpu, init_cpu, FULL_SEED)
    _, g32 = full_reference(llh, torch.float32, Z_cpu, init_cpu, FULL_SEED)
    out_gate(f"full model, SiLU denoiser {llh}", out, o64)
    for k, t in zip(("y", "kernel", "alpha"), ins):
        gate(f"full model, SiLU denoiser {llh} d/d{k}", t.grad, g32[k], g64[k])


# ----------------------------------------------------------------------------- 6. determinism, chunking, routing
@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_chunked_and_repeated_runs_are_bit_identical(dev, llh):
    from gdeconv import _lib
    lib = _lib.load()
    case = (64, 64, 48, 7, 2, "per_galaxy")       # compares no reference: no kink condition
    per_galaxy_ws = 2 * 33 * 64 * 8
    old_b = lib.gd_set_chunk_bytes(0)
    old_s = lib.gd_set_pipeline_streams(3)
    old_f = lib.gd_set_fused_iteration(1)
    try:
        one, g_one = loop_engine(case, llh, dev, True)                # one pass over the batch
        again, g_again = loop_engine(case, llh, dev, True)
        lib.gd_set_chunk_bytes(3 * per_galaxy_ws)                     # chunks of 3, 3, 1 galaxies on 3 streams
        chunked, g_chunked = loop_engine(case, llh, dev, True)
        lib.gd_set_chunk_bytes(0)
        lib.gd_set_fused_iteration(0)                                 # the routing switches do not reach training
        unfused, g_unfused = loop_engine(case, llh, dev, True)
    finally:
        lib.gd_set_chunk_bytes(old_b)
        lib.gd_set_pipeline_streams(old_s)
        lib.gd_set_fused_iteration(old_f)
    assert torch.isfinite(one).all()
    for o, g in ((again, g_again), (chunked, g_chunked), (unfused, g_unfused)):
        assert torch.equal(one, o)
        for k in g_one:
            assert torch.isfinite(g_one[k]).all(), k
            assert torch.equal(g_one[k], g[k]), k


# ----------------------------------------------------------------------------- 7. no regression by construction
@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_without_input_grads_it_is_the_trainable_class(dev, llh):
    from gdeconv.models import TrainableUnrolledADMM
    case = LOOP_CASES[0]
    a, ga = loop_engine(case, llh, dev, True, wrt=())
    b, gb = loop_engine(case, llh, dev, True, wrt=(), cls=TrainableUnrolledADMM)
    assert torch.equal(a, b)
    for k in ("rho1", "rho2", "weight", "scale"):
        assert torch.equal(ga[k], gb[k]), k
    for k in ("y", "kernel", "alpha"):
        assert ga[k] is None


@pytest.mark.parametrize("llh", ["Poisson", "Gaussian"])
def test_no_grad_is_the_inference_path(dev, llh):
    from gdeconv.models import DifferentiableUnrolledADMM, Unrolled_ADMM
    from gdeconv.weights import make_state_dict
    a = Unrolled_ADMM(n_iters=3, llh=llh)
    a.load_state_dict(make_state_dict(a, 77))
    b = DifferentiableUnrolledADMM(n_iters=3, llh=llh)
    b.load_state_dict(a.state_dict())
    a.Z, b.Z = torch.nn.Identity(), torch.nn.Identity()
    a, b = a.to(dev).eval(), b.to(dev).eval()
    y, psf, alpha, _ = make_batch(3, 48, h=48, seed=9)
    y, psf, alpha = y.to(dev), psf.to(dev).requires_grad_(), alpha.to(dev)
    with torch.no_grad():
        oa, ob = a(y, psf.detach(), alpha), b(y, psf, alpha)
    assert not ob.requires_grad
    assert torch.equal(oa, ob)
