#!/usr/bin/env python
"""Time one training step (forward + backward) of the unrolled-ADMM spectral path, with a cheap conv denoiser:

  engine   ``TrainableUnrolledADMM``: every loop body one gd_admm_train_iter, its adjoint gd_admm_train_iter_backward
  torch    the same loop restated with ``torch.fft.rfft2`` on the GPU under autograd (``torch_loop`` below; the
           baseline a user has without the engine's backward)

in ONE process, in interleaved blocks (engine, torch, engine, torch, ...) after a warm-up of both, the median block
per path.  The two outputs and rho gradients are compared in the same run.  Prints one JSON line per (shape,
likelihood) and writes them all to ``--out``.

    python tools/train_step_bench.py --out profiles/train_step_bench.json

``--input-grads``: the same step with y, the PSF and alpha requiring grad as well (``DifferentiableUnrolledADMM``:
gd_admm_train_iter_full and its adjoint, the HIP adjoints of psf_to_otf and conv_fft_batch) against the same
``rfft2`` loop differentiating its inputs; the parameter-only engine step is re-measured in the same interleaved
blocks, so the record also holds what the input gradients cost on top of it.

    python tools/train_step_bench.py --input-grads --out profiles/train_step_bench_input_grads.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "galaxy-deconv_amd"))

from gdeconv.models import DifferentiableUnrolledADMM, TrainableUnrolledADMM  # noqa: E402
from gdeconv.synth import make_batch  # noqa: E402


class ConvDenoiser(torch.nn.Module):
    def __init__(self):
        super().__init__()
        w = 0.05 * torch.randn(1, 1, 3, 3, generator=torch.Generator().manual_seed(11))
        w[0, 0, 1, 1] += 1.0
        self.weight = torch.nn.Parameter(w)
        self.scale = torch.nn.Parameter(torch.tensor(0.9))

    def forward(self, x):
        return F.conv2d(x, self.weight, padding=1) * self.scale


def torch_loop(y, psf, alpha, rho1, rho2, llh, den):
    """models/Unrolled_ADMM.py:177-215 with real FFTs (one conv(H, x) per iteration, reused by the dual update and
    the next V step)."""
    N, _, H, W = y.shape
    rf, irf = torch.fft.rfft2, (lambda s: torch.fft.irfft2(s, s=(H, W)))
    h = psf.shape[-1]
    placed = torch.roll(F.pad(psf, (0, W - h, 0, H - h)), shifts=(-(h // 2), -(h // 2)), dims=(2, 3))
    Hf = rf(placed)
    Ht, HtH = Hf.conj(), Hf.abs() ** 2
    yp = y.clamp_min(0)

    def V(vt, r):
        if llh == "Poisson":
            t = r * vt - alpha
            return 0.5 * (1 / r) * (-t + torch.sqrt(t ** 2 + 4 * yp * r))
        return (r * vt + yp / alpha) / (1 + r)

    x = irf(Ht * rf(yp / alpha) / (HtH + 1 / alpha)).clamp(0, 1)
    u1, u2, hx = torch.zeros_like(x), torch.zeros_like(x), irf(Hf * rf(x))
    for i in range(rho1.shape[0]):
        v = V(hx + u2, rho2[i])
        z = den(x + u1)
        x = irf((rho1[i] * rf(z - u1) + rho2[i] * Ht * rf(v - u2)) / (rho1[i] * HtH + rho2[i]))
        hx = irf(Hf * rf(x))
        u1, u2 = u1 + x - z, u2 + hx - v
    return x * alpha if llh == "Poisson" else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x48,64x256", help="comma-separated NxL")
    ap.add_argument("--n-iters", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10, help="training steps per timed block")
    ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per path (median reported)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--input-grads", action="store_true", help="y, psf and alpha require grad as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_step_bench needs a ROCm device (no CPU timing)")
    dev = torch.device("cuda:0")
    from gdeconv import _lib
    rev = _lib.load().gd_engine_rev().decode()
    results = []
    for shape in a.shapes.split(","):
        N, L = (int(t) for t in shape.split("x"))
        y, psf, alpha, _ = make_batch(N, L, h=min(48, L), seed=1, device=dev)
        R = torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).to(dev)
        for llh in ("Poisson", "Gaussian"):
            m = (DifferentiableUnrolledADMM if a.input_grads else TrainableUnrolledADMM)(
                n_iters=a.n_iters, llh=llh, subnet=False)
            m.Z = ConvDenoiser()
            m = m.to(dev).train()
            with torch.no_grad():
                g = torch.Generator().manual_seed(3)
                m.rho1_iters.copy_(0.5 + torch.rand(a.n_iters, generator=g))
                m.rho2_iters.copy_(0.5 + torch.rand(a.n_iters, generator=g))

            leaves = [t.clone().requires_grad_() for t in (y, psf, alpha)] if a.input_grads else []

            def step(engine, inputs=a.input_grads):
                m.zero_grad(set_to_none=True)
                for t in leaves:
                    t.grad = None
                yy, pp, aa = leaves if inputs else (y, psf, alpha)
                out = m(yy, pp, aa) if engine else torch_loop(yy, pp, aa, m.rho1_iters, m.rho2_iters, llh, m.Z)
                (out * R).sum().backward()
                return (out.detach(), m.rho1_iters.grad.clone(), m.rho2_iters.grad.clone(),
                        *([t.grad.clone() for t in leaves] if inputs else []))

            def block(engine):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    step(engine)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / a.steps

            def block_params_only():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    step(True, inputs=False)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / a.steps

            for _ in range(a.warmup):
                re_ = step(True)
                rt_ = step(False)
                if a.input_grads:
                    step(True, inputs=False)
            rel = lambda p, q: float((p - q).abs().max() / q.abs().max())  # noqa: E731
            names = ["out", "d_rho1", "d_rho2"] + (["d_y", "d_psf", "d_alpha"] if a.input_grads else [])
            agree = {k: rel(p, q) for k, p, q in zip(names, re_, rt_)}
            te, tt, tp = [], [], []
            for _ in range(a.blocks):
                te.append(block(True))
                tt.append(block(False))
                if a.input_grads:
                    tp.append(block_params_only())
            rec = {"tool": "train_step_bench", "engine_rev": rev, "N": N, "H": L, "W": L, "llh": llh,
                   "n_iters": a.n_iters, "steps_per_block": a.steps, "blocks": a.blocks,
                   "engine_ms_per_step": statistics.median(te), "torch_rfft2_ms_per_step": statistics.median(tt),
                   "engine_ms_blocks": te, "torch_rfft2_ms_blocks": tt,
                   "speedup": statistics.median(tt) / statistics.median(te), "engine_vs_torch_max_rel": agree}
            if a.input_grads:
                rec.update({"input_grads": True, "engine_params_only_ms_per_step": statistics.median(tp),
                            "engine_params_only_ms_blocks": tp,
                            "input_grads_cost_ratio": statistics.median(te) / statistics.median(tp)})
            print(json.dumps(rec), flush=True)
            assert max(agree.values()) < 1e-3, f"the two paths disagree: {agree}"
            results.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
