"""Host mirror of the averaged generator's recurrence (csrc/adam.hip: ema_one_minus_decay / ema_one; include/pdgn_hip.h,
pdgn_adam_ema_multi): numpy only, the arithmetic the header fixes, so that tests can demand equal bits.

    d_t = min(ema_decay, (1 + t) / (10 + t))      float64, t the step count of the update that produced p
    omd = float32(1 - d_t)
    e   = e + omd * (p - e)                       three separately rounded float32 operations (one numpy ufunc each)
"""
import numpy as np


def decay_at(ema_decay, t):
    return min(np.float64(ema_decay), (np.float64(1.0) + np.float64(t)) / (np.float64(10.0) + np.float64(t)))


def one_minus_decay(ema_decay, t):
    return np.float32(np.float64(1.0) - decay_at(ema_decay, t))


def ema_update(e, p, ema_decay, t):
    """One update; e, p: float32 arrays of one shape.  Returns the new average (float32)."""
    e, p = np.asarray(e), np.asarray(p)
    assert e.dtype == np.float32 and p.dtype == np.float32 and e.shape == p.shape
    omd = one_minus_decay(ema_decay, t)
    diff = np.subtract(p, e, dtype=np.float32)
    scaled = np.multiply(omd, diff, dtype=np.float32)
    return np.add(e, scaled, dtype=np.float32)


def ema_run(e0, snapshots, ema_decay, t0):
    """The recurrence over parameter snapshots taken after the updates t0, t0 + 1, ..."""
    e = np.asarray(e0, dtype=np.float32)
    for i, p in enumerate(snapshots):
        e = ema_update(e, p, ema_decay, t0 + i)
    return e
