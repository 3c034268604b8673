"""The training loop behind `PDGNTrainer.fit` (models/PDGNet_v2.py:157-269) and its host-side parts: the side logs
(grad_norms.csv, lr.csv, aug.csv, repulsion.csv, flatness.csv), the two-slot read-back of the losses, and the gradient guard's stop rule.

Everything here takes the trainer as an argument and asks it only for what the feature in use needs, so `fit` also runs on a
duck-typed stand-in without `guards`, `lr_table`, `per_network_lr`, `aug`, `repulsion` or `flatness` (tests/test_fit_host.py).  This module imports
nothing from `trainer`; `trainer` re-exports the names below that were defined there.
"""
import contextlib
import os
import time

import torch

LOG_FORMAT = ("Epoch: [%2d] [%4d/%4d] time: %2dm %2ds d_loss1: %.8f d_loss2: %.8f d_loss3: %.8f d_loss4: %.8f, "
              "g_loss: %.8f, similar_loss: %.8f")         # :259
LOSS_KEYS = ("d_loss1", "d_loss2", "d_loss3", "d_loss4", "g_loss", "similar_loss")
GUARD_KEYS = ("G", "D1", "D2", "D3", "D4")
GUARD_RECORD_FLOATS = 8             # sizeof(pdgn_guard_record) / 4 (include/pdgn_hip.h): norm, coef, applied, found_inf, two counters, two spare


class GradGuardError(RuntimeError):
    """`fit` saw `guard_max_skips` consecutive skipped updates of a network: its gradients have stopped being finite."""


def decode_guard_record(words):
    """{norm, coef, applied, skipped} from the 8 words of a record read back as fp32 (a host tensor): the two counters are
    the running numbers of applied and skipped updates."""
    ints = words.contiguous().view(torch.int32)
    return {"norm": float(words[0]), "coef": float(words[1]), "applied": int(ints[4]) & 0xffffffff, "skipped": int(ints[5]) & 0xffffffff}


def _is_path(log):
    return isinstance(log, (str, bytes, os.PathLike))


class SideLog:
    """One CSV file beside the training log, appended to: `path`, or else `name` in the directory of `beside` where that is a
    path (the log; a callable log has no directory).  The header is written exactly when the file is missing or empty.  Without
    a path, or with active=False (the feature is off, or this is not rank 0), no file is made and every call does nothing."""

    def __init__(self, path, header, beside=None, name=None, active=True):
        if path is None and name is not None and _is_path(beside):
            path = os.path.join(os.path.dirname(os.fspath(beside)) or ".", name)
        self._file, self._key = None, None
        if active and path is not None:
            fresh = not os.path.exists(path) or os.path.getsize(path) == 0
            self._file = open(path, "a")
            if fresh:
                self._file.write(",".join(header) + "\n")

    def row(self, fields, key=None):
        """Write and flush the row `fields()` (a list of strings; not called when nothing is written).  With a key, a row
        whose key is that of the previous keyed row is left out."""
        if self._file is None or (key is not None and key == self._key):
            return
        self._key = key if key is not None else self._key
        self._file.write(",".join(fields()) + "\n")
        self._file.flush()

    def close(self):
        if self._file is not None:
            self._file.close()
            self._file = None


def _last_skipped(rec):
    """Whether the record's LAST gradient list was not finite (norm is Inf or NaN exactly then)."""
    return not (rec["norm"] == rec["norm"] and abs(rec["norm"]) != float("inf"))


class SkipWatch:
    """The guard's stop rule: per network, the number of consecutive lines in which its skipped counter rose; at `max_skips`,
    a checkpoint of the current epoch (`save_to`: the directory, or None) and GradGuardError."""

    def __init__(self, trainer, max_skips, norms, save_to, category):
        self.trainer, self.max_skips, self.norms, self.save_to, self.category = trainer, int(max_skips), norms, save_to, category
        self.skipped_before, self.run_of_skips = None, [0] * len(GUARD_KEYS)

    def one_short(self):
        return max(self.run_of_skips) >= self.max_skips - 1

    def line(self, ep, idx, recs):
        self.norms.row(lambda: ["%d" % ep, "%d" % (idx + 1)] + ["%.9g" % r[f] for r in recs for f in ("norm", "coef")]
                       + ["%d" % sum(r["skipped"] for r in recs)])
        now, run = [r["skipped"] for r in recs], self.run_of_skips
        if self.skipped_before is not None:                      # (the first line has nothing to compare with: capture_list's warm-up
            for i in range(len(run)):                            #  iterations, an earlier fit, have counted too)
                run[i] = run[i] + 1 if now[i] != self.skipped_before[i] else 0
        else:
            for i in range(len(run)):
                run[i] = 1 if recs[i]["applied"] + recs[i]["skipped"] > 0 and _last_skipped(recs[i]) else 0
        self.skipped_before = now
        worst = max(range(len(run)), key=lambda i: run[i])
        if run[worst] >= self.max_skips:
            where = ""
            if self.save_to is not None:
                where = "; checkpoint of the last finite parameters: " + self.trainer.save(self.save_to, ep, self.category)[0]
            raise GradGuardError("gradient guard: %s skipped %d consecutive updates (epoch %d, iteration %d): its gradients are "
                                 "not finite%s" % (GUARD_KEYS[worst], run[worst], ep, idx + 1, where))


class LossReadback:
    """The losses (and, with a guard, the five records behind them) of every iteration, copied non-blocking into one of two
    host rows (pinned on a CUDA device) behind an event each: the line of iteration n is written after iteration n + 1 has
    been issued, when that copy is long complete -- or at once, when the watch says a network is one skip short of the end,
    so that no further iteration is issued."""

    def __init__(self, trainer, nb, sink, watch):
        self.trainer, self.nb, self.sink, self.watch = trainer, nb, sink, watch
        self.cuda = trainer.device.type == "cuda"
        self.nl = len(trainer.LOSS_KEYS)
        width = self.nl + (len(GUARD_KEYS) * GUARD_RECORD_FLOATS if watch is not None else 0)
        self.host = torch.empty(2, width, dtype=torch.float32, pin_memory=self.cuda)
        self.done = [torch.cuda.Event() for _ in range(2)] if self.cuda else None
        self.pending, self.n, self.start = None, 0, time.time()

    def push(self, epoch, i, out):
        tr, slot = self.trainer, self.n & 1
        row = torch.stack([out[k] for k in tr.LOSS_KEYS])
        self.host[slot].copy_(torch.cat([row, tr.guard_buf.view(-1)]) if self.watch is not None else row, non_blocking=True)
        if self.cuda:
            self.done[slot].record(torch.cuda.current_stream(tr.device))
        self.flush()
        self.pending = (slot, epoch, i)
        self.n += 1
        if self.watch is not None and self.watch.one_short():
            self.flush()                                         # one skip short of the end: this iteration's line now, not behind the next

    def flush(self):
        if self.pending is None:
            return
        (slot, ep, idx), self.pending = self.pending, None
        if self.cuda:
            self.done[slot].synchronize()
        dt = time.time() - self.start
        row, nl, w = self.host[slot], self.nl, GUARD_RECORD_FLOATS
        if self.sink is not None:
            self.sink(self.trainer.LOG_FORMAT % ((ep, idx + 1, self.nb, dt / 60, dt % 60) + tuple(row[:nl].tolist())))
        if self.watch is not None:
            self.watch.line(ep, idx, [decode_guard_record(row[nl + i * w:nl + (i + 1) * w]) for i in range(len(GUARD_KEYS))])


def _rates_row(trainer, ep):
    state = trainer.lr_state()
    return ["%d" % ep, "%d" % state["G"]["step"]] + ["%.17g" % state[k]["lr"] for k in GUARD_KEYS]


def _ada_row(trainer, ep):
    state = trainer.aug_state()
    a = state["ada"]
    per = [(ps - ng) / n if n else float("nan") for ps, ng, n in a["last_net"]]
    return ["%d" % ep, "%d" % state["clock"], "%.17g" % a["p"], "%d" % a["updates"], "%.17g" % a["last_r"]] + ["%.17g" % r for r in per]


def _repulsion_row(trainer, ep):
    state = trainer.repulsion_state()
    return ["%d" % ep, "%.9g" % state["weight"], "%.9g" % state["radius"], "%.9g" % state["total"]] + ["%.9g" % v for v in state["per_level"]]


def _flatness_row(trainer, ep):
    state = trainer.flatness_state()
    return (["%d" % ep, "%.9g" % state["weight"], "%d" % state["k"], "%.9g" % state["eps"], "%.9g" % state["total"]]
            + ["%.9g" % v for v in state["per_level"]] + ["%d" % state["degenerate"]])


def fit(trainer, feeder, epochs, start_epoch=1, snapshot=20, checkpoint_dir=None, category="chair", issue="list", log=None,
        on_epoch=None, guard_max_skips=50, grad_norms=None, lr_log=None, aug_log=None, repulsion_log=None, flatness_log=None):
    """`PDGNTrainer.fit`: its docstring is the contract."""
    if issue not in ("list", "eager"):
        raise ValueError("issue: 'list' or 'eager', got %r" % (issue,))
    guarded = getattr(trainer, "guards", None) is not None
    if guarded and int(guard_max_skips) < 1:
        raise ValueError("guard_max_skips must be at least one, got %r" % (guard_max_skips,))
    rank0 = getattr(feeder, "rank", 0) == 0
    save_to = checkpoint_dir if rank0 else None
    aug = getattr(trainer, "aug", None)
    scheduled = getattr(trainer, "lr_table", None) is not None or getattr(trainer, "per_network_lr", False)
    nb = feeder.batches_per_epoch
    with contextlib.ExitStack() as files:
        sink = log
        if _is_path(log):
            opened = files.enter_context(open(log, "a"))
            sink = lambda line: (opened.write(line + "\n"), opened.flush())

        def side(path, name, on, header):
            return files.enter_context(contextlib.closing(SideLog(path, header, beside=log, name=name, active=on and rank0)))

        norms = side(grad_norms, "grad_norms.csv", guarded,
                     ["epoch", "iter"] + ["%s_%s" % (k, f) for k in GUARD_KEYS for f in ("norm", "coef")] + ["skipped_total"])
        rates = side(lr_log, "lr.csv", scheduled, ["epoch", "step_G"] + ["lr_%s" % k for k in GUARD_KEYS])
        ada = side(aug_log, "aug.csv", aug is not None and aug.adaptive is not None,
                   ["epoch", "clock", "p", "updates", "last_r"] + ["r_%s" % k for k in GUARD_KEYS[1:]])

        repel = side(repulsion_log, "repulsion.csv", getattr(trainer, "repulsion", None) is not None,
                     ["epoch", "weight", "radius", "total"] + ["level%d" % l for l in (1, 2, 3, 4)])
        flat = side(flatness_log, "flatness.csv", getattr(trainer, "flatness", None) is not None,
                    ["epoch", "weight", "k", "eps", "total"] + ["level%d" % l for l in (1, 2, 3, 4)] + ["degenerate"])

        def epoch_rows(ep):                                      # one row per epoch: the last epoch's checkpoint may be written twice
            ada.row(lambda: _ada_row(trainer, ep), key=ep)
            rates.row(lambda: _rates_row(trainer, ep), key=ep)

        watch = SkipWatch(trainer, guard_max_skips, norms, save_to, category) if guarded else None
        back = LossReadback(trainer, nb, sink, watch) if sink is not None or guarded else None

        if issue == "eager" or getattr(trainer, "_list", None) is None:
            reals, z1, z2 = feeder.buffers()
        if issue == "list" and getattr(trainer, "_list", None) is None and start_epoch <= epochs:
            feeder.fill(start_epoch, 0, reals, z1, z2)
            trainer.capture_list(reals, z1, z2)
        if issue == "list":
            st = trainer._static
            reals, z1, z2 = st["reals"], st["z1"], st["z2"]
        if aug is not None:
            # iteration i of epoch e always draws at (e - 1) * nb + i, the feeder's global iteration: set behind capture_list's
            # warm-up iterations (they tick too), so that a resumed epoch draws what the uninterrupted run drew
            aug.set_clock((start_epoch - 1) * nb)
        for epoch in range(start_epoch, epochs + 1):
            for i in range(nb):
                feeder.fill(epoch, i, reals, z1, z2)
                out = trainer.step_list() if issue == "list" else trainer.step(reals, z1, z2)
                if back is not None:
                    back.push(epoch, i, out)
            if save_to is not None and epoch % snapshot == 0:
                trainer.save(save_to, epoch, category)
                epoch_rows(epoch)
            if on_epoch is not None:
                on_epoch(epoch)
                epoch_rows(epoch)
            repel.row(lambda: _repulsion_row(trainer, epoch), key=epoch)     # every epoch: the last iteration's values (one synchronise)
            flat.row(lambda: _flatness_row(trainer, epoch), key=epoch)
        if back is not None:
            back.flush()
        if save_to is not None:
            trainer.save(save_to, epochs, category)              # (:268: always, whatever the snapshot period)
            epoch_rows(epochs)
    return epochs
