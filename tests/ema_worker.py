"""The averaged generator inside a small trainer, against the host mirror (tests/ema_mirror.py): shared by tests/test_gpu_ema.py and
its child process (python tests/ema_worker.py, run there with PDGN_OWN_ADAM=0 so that the optimizer step is torch's kernel and the
average the stand-alone launch)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ema_mirror as em  # noqa: E402

DECAY = 0.999


def trainer_scenario(eager_steps=3, list_steps=3):
    """B = 4, ema_decay = 0.999: `eager_steps` eager steps, capture_list (its warm-up iterations are real updates), `list_steps`
    replays.  The generator's parameters are cloned behind EVERY optimizer update -- eager and warm-up updates by a wrapper around
    the generator's optimizer step (inactive while the stream is capturing: nothing is added to the list), replays after each
    step_list() -- and the average must be, bit for bit, the mirror's recurrence over those snapshots: a statement about the
    average given the parameters, whatever the step's own float atomics made of them.  Returns (trainer, reals, z1, z2)."""
    from pdgn_amd.trainer import PDGNTrainer, noise, synthetic_batch
    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    tr = PDGNTrainer(device=dev, distributed=False, ema_decay=DECAY)
    tr.train()
    params = tr.optG.param_groups[0]["params"]
    assert tr.ema is not None and len(tr.ema) == len(params) and tr.ema_buf.dtype == torch.float32
    assert all(e.shape == p.shape and e.data_ptr() % 16 == 0 and torch.equal(e, p) for e, p in zip(tr.ema, params))
    e0 = [e.detach().cpu().numpy().copy() for e in tr.ema]
    snaps = []

    def snapshot():
        snaps.append([p.detach().clone() for p in params])

    inner = tr._stepG.step

    def step_and_snapshot():
        inner()
        if not torch.cuda.is_current_stream_capturing():
            snapshot()

    tr._stepG.step = step_and_snapshot
    B = 4
    reals, z1, z2 = synthetic_batch(B, dev), noise(B, dev), noise(B, dev)

    def adam_step():
        return float(tr.optG.state[params[0]]["step"])

    def check(label):
        torch.cuda.synchronize()
        assert len(snaps) == adam_step(), (label, len(snaps), adam_step())       # every update was seen, warm-up ones included
        for i, (e, start) in enumerate(zip(tr.ema, e0)):
            want = em.ema_run(start, [s[i].cpu().numpy() for s in snaps], DECAY, 1)
            got = e.detach().cpu().numpy()
            assert np.array_equal(got, want), (label, i, float(np.abs(got - want).max()))
        # (not a vacuous statement: the average moved, and is not the parameters)
        assert any(not np.array_equal(e.detach().cpu().numpy(), s) for e, s in zip(tr.ema, e0))
        assert any(not torch.equal(e, p) for e, p in zip(tr.ema, params))

    for _ in range(eager_steps):
        tr.step(reals, z1, z2)
    check("eager")
    tr.capture_list(reals, z1, z2)
    assert adam_step() > eager_steps                                             # the warm-up iterations are real updates
    check("capture")
    tr._stepG.step = inner
    for _ in range(list_steps):
        out = tr.step_list(None, z1, z2)
        torch.cuda.synchronize()
        snapshot()
    assert all(torch.isfinite(v).item() for v in out.values())
    check("list")
    own = os.environ.get("PDGN_OWN_ADAM", "1") == "1"
    assert (tr._stepG.route == "own") == own                                     # which optimizer kernel ran
    return tr, reals, z1, z2


if __name__ == "__main__":
    tr = trainer_scenario()[0]
    tr._list, tr._list_points, tr._static = None, [], None
    torch.cuda.synchronize()
    print("ema worker ok: PDGN_OWN_ADAM=%s, %d updates" % (os.environ.get("PDGN_OWN_ADAM", "1"),
                                                          int(tr.optG.state[tr.optG.param_groups[0]["params"][0]]["step"])))
