"""The gradient guard behind trainer.LeanAdamStep on a plain tensor list: shared by tests/test_gpu_gradguard.py and its child process
(python tests/gradguard_worker.py, run there with PDGN_OWN_ADAM=0 so that every optimizer step is torch's kernel with the guard's flag
as its `found_inf`, the gradients scaled in place, and the average the guarded stand-alone launch)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# the list of test_own_adam_kernel_equals_torch_fused_adam's kind: one element, not a multiple of 4, the chunk boundary (4096) from
# both sides, several chunks, a ragged large one, and 80 small ragged tensors -- 89 tensors, more than one Adam launch carries (72 / 64)
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 12288, 100003] + [17 + 13 * i for i in range(80)]
I_4097, I_1 = SIZES.index(4097), SIZES.index(1)


def magnitudes(seed=0):
    """One magnitude per tensor, spread log-uniformly over 1e-4 .. 1e2."""
    g = torch.Generator().manual_seed(seed)
    return [float(10.0 ** (-4.0 + 6.0 * torch.rand((), generator=g))) for _ in SIZES]


def lean_scenario(poison_at=3, steps=5):
    """Two copies of the list, each with torch's fused capturable Adam, an average and a guard (no clipping) behind LeanAdamStep, and a
    third with neither; `steps` steps on the same gradients, the second copy with one NaN in its gradients at step `poison_at`.
    Checks what the guard promises and returns the number of applied updates of the poisoned copy."""
    from pdgn_amd.trainer import GradGuard, LeanAdamStep, PDGNTrainer
    dev = torch.device("cuda:0")
    mags = magnitudes()

    def make(guarded=True):
        gen = torch.Generator(device=dev).manual_seed(1)
        params = [torch.nn.Parameter(torch.randn(n, device=dev, generator=gen)) for n in SIZES]
        opt = torch.optim.Adam(params, lr=1e-4, betas=(0.5, 0.999), capturable=True, fused=True)
        if not guarded:
            return params, opt, None, None, LeanAdamStep(opt)
        ema = PDGNTrainer._flat_like(params)[1]
        with torch.no_grad():
            torch._foreach_copy_(ema, [p.detach() for p in params])
        guard = GradGuard(params)
        return params, opt, ema, guard, LeanAdamStep(opt, ema, 0.999, guard)

    def state(params, opt, ema):                                 # parameters and averages first, then whatever Adam state exists
        out = [p.detach().clone() for p in params] + [e.clone() for e in ema]
        for p in params:
            out += [opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq", "step") if p in opt.state]
        return out

    clean, bad, plain = make(), make(), make(guarded=False)
    applied = 0
    for t in range(1, steps + 1):
        gen = torch.Generator(device=dev).manual_seed(100 + t)
        grads = [torch.randn(n, device=dev, generator=gen) * m for n, m in zip(SIZES, mags)]
        for copy in (clean, bad, plain):
            params, opt, ema, guard, lean = copy
            poisoned = copy is bad and t == poison_at
            for i, (p, g) in enumerate(zip(params, grads)):
                p.grad = g.clone()
                if poisoned and i == I_4097:
                    p.grad[-1] = float("nan")
            before = state(params, opt, ema) if poisoned else None
            lean.step()
            torch.cuda.synchronize()
            if copy is not bad:
                continue
            assert all(torch.isfinite(e).all().item() for e in ema), ("the average", t)
            if poisoned:                                         # byte-identical to the state after the step before
                after = state(params, opt, ema)
                assert all(torch.equal(a, b) for a, b in zip(before, after)), ("a skipped update wrote", t)
                if len(before) < len(after):                     # (the optimizer's FIRST step creates its state: zeros, and they stay zeros)
                    assert not any(x.any().item() for x in after[len(before):])
                rec = guard.state()
                assert rec["skipped"] == 1 and rec["applied"] == applied and rec["norm"] != rec["norm"] and rec["coef"] == 1.0
            else:
                applied += 1
            assert all(float(opt.state[p]["step"]) == applied for p in params), ("step counters", t, applied)
    assert applied == steps - 1 and bad[3].state()["applied"] == applied
    assert all(float(clean[1].state[p]["step"]) == steps for p in clean[0])
    rec = clean[3].state()
    assert rec["applied"] == steps and rec["skipped"] == 0 and rec["coef"] == 1.0 and rec["norm"] > 0
    own = os.environ.get("PDGN_OWN_ADAM", "1") == "1"
    assert (clean[4].route == "own") == own and (bad[4].route == "own") == own      # which optimizer kernel ran
    # a guard that neither clips nor skips is the unguarded optimizer, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(clean[0], plain[0]))
    assert all(torch.equal(clean[1].state[a][k], plain[1].state[b][k]) for a, b in zip(clean[0], plain[0]) for k in ("exp_avg", "exp_avg_sq"))
    return applied


if __name__ == "__main__":
    for at in (3, 1):
        n = lean_scenario(poison_at=at)
        print("gradguard worker ok: PDGN_OWN_ADAM=%s, poisoned step %d, %d of 5 applied" % (os.environ.get("PDGN_OWN_ADAM", "1"), at, n))
