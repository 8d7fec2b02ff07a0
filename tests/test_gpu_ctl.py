"""GPU: the two Gram forms of the device-side Arnoldi control give the same bits.

The control of one Arnoldi step (csrc/arnctl_dev.h ctl_run) is written once and takes the stored
Gram rows either through LDS (GramLds: the control launch and the fused launches' tail) or from
registers (GramRegs: the reduce + control launches, the default one-GPU path).  Both must run the
MGS forward substitution on the same values in the same order.  nk_debug_ctl_step runs one step
on a synthetic state through the solver's own launch of either form; the state after the step,
its host mirror and the fused step's parameter block are compared byte for byte, never to a
tolerance.

Steps: t = 1 (no previous rotation, no stored Gram row), 2 (the first with both), 3, 17, and 34,
the last step the device may take (t + 1 <= nv_max <= kArnMaxNV = 35: the last iteration of the
unrolled register loop, Gram row 33), each with an exact scale (sig_est = 0) and a lagged one
(0.9 of the scale 1/|V_t| the step computes).  |h|^2 is about 0.01 (t + 1) against |w|^2 >= 4,
so these steps continue; every reason to hand a step back is then taken once at t = 17.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_ARN_MAX_NV = 35      # csrc/nk_kernels.h kArnMaxNV
K_LAG_MIN_RATIO2 = 1e-12  # csrc/lgmres.cpp kLagMinRatio2
HALT = K_ARN_MAX_NV + 3   # the parameter block's entry "the queued fused step does nothing"


def _case(t, lagged, seed):
    rng = np.random.default_rng([2020, t, seed])
    n = t + 1
    red = np.empty(2 * n + 1)
    red[:n] = rng.uniform(-0.1, 0.1, n)            # w . V_i
    red[n:n + t] = rng.uniform(-1e-3, 1e-3, t)     # V_t . V_i
    red[n + t] = rng.uniform(0.5, 2.0)             # |V_t|^2
    red[2 * n] = 4.0                               # |w|^2
    ang = rng.uniform(0.0, 2.0 * np.pi, t)
    return {
        "t": t,
        # j, hn_pending, m, nv_max, halt, steps
        "ints": np.array([t, 1, t + 5, max(t + 1, K_ARN_MAX_NV), 0, 3], dtype=np.int32),
        # wnorm[t-1], gv[t-1], sig_est[t], ptol, omega, lag_ratio2
        "scal": np.array([1.0, 0.3, 0.9 / np.sqrt(red[n + t]) if lagged else 0.0, 1e-300, 1e-6,
                          K_LAG_MIN_RATIO2]),
        "sig": rng.uniform(0.5, 2.0, n),
        "h": rng.uniform(-1.0, 1.0, t),
        "cs": np.cos(ang),
        "sn": np.sin(ang),
        "gram": rng.uniform(-1e-3, 1e-3, (t, t)),
        "red": red,
    }


def _run(form, c):
    from nkhip import _lib
    nbytes = _lib.lib.nk_debug_ctl_step(0, 0, *([None] * 12))
    assert nbytes > 0
    state, mirror = np.zeros(nbytes, np.uint8), np.zeros(nbytes, np.uint8)
    prm = np.full(K_ARN_MAX_NV + 4, np.nan)
    status = C.c_uint32(99)
    arrs = [np.ascontiguousarray(c[k]) for k in ("ints", "scal", "sig", "h", "cs", "sn", "gram",
                                                 "red")]
    rc = _lib.lib.nk_debug_ctl_step(form, c["t"], *[a.ctypes.data for a in arrs],
                                    state.ctypes.data, mirror.ctypes.data, prm.ctypes.data,
                                    C.addressof(status))
    assert rc == 0, f"nk_debug_ctl_step rc={rc}"
    return state.tobytes(), mirror.tobytes(), prm, status.value


def _both(c):
    a, b = _run(0, c), _run(1, c)
    for what, x, y in zip(("device state", "host mirror"), a[:2], b[:2]):
        assert x == y, f"{what} differs between the LDS and the register form"
    assert a[2].tobytes() == b[2].tobytes(), f"parameter block: {a[2]} != {b[2]}"
    assert a[3] == b[3]
    for form, r in enumerate((a, b)):  # (the arrival counters are back to zero with it)
        assert r[0] == r[1], f"form {form}: device state and host mirror differ"
    return a


@pytest.mark.parametrize("lagged", [False, True])
@pytest.mark.parametrize("t", [1, 2, 3, 17, 34])
def test_continuing_step_same_bits(t, lagged):
    c = _case(t, lagged, 0)
    state, _, prm, status = _both(c)
    assert status == 1
    assert prm[HALT] == 0.0
    assert np.all(np.isfinite(prm))
    assert np.all(prm[t + 1:K_ARN_MAX_NV] == 0.0) and np.any(prm[:t + 1] != 0.0)
    if lagged:
        assert abs(prm[K_ARN_MAX_NV] - 1.0 / 0.9) < 1e-12  # tau = sig_t / sig_est[t]
    else:
        assert prm[K_ARN_MAX_NV] == 1.0


def _set(field, i, v):
    def f(c):
        c[field][i] = v
    return f


T_HB = 17
HAND_BACKS = {
    "other_step": _set("ints", 0, T_HB - 1),          # j != t
    "norm_not_pending": _set("ints", 1, 0),           # hn_pending = 0
    "basis_full": _set("ints", 3, T_HB),              # nv_max = t
    "last_step": _set("ints", 2, T_HB + 1),           # m = t + 1
    "converged": _set("scal", 3, 1.0),                # ptol = 1 > |gv_next|
    "breakdown": _set("red", 2 * T_HB + 1, 0.0),      # |V_t|^2 = 0
    "nonfinite_w": _set("red", 2 * T_HB + 2, np.inf),
    "cancelled_estimate": _set("red", 2 * T_HB + 2, 1e-30),  # |w|^2 - |h|^2 < 0
}


@pytest.mark.parametrize("why", list(HAND_BACKS))
def test_hand_back_same_bits(why):
    c = _case(T_HB, False, 1)
    HAND_BACKS[why](c)
    _, _, prm, status = _both(c)
    assert status == 2
    assert prm[HALT] == 1.0
    assert np.all(np.delete(prm, HALT) == 0.0)  # no parameters of a step that does not run


def test_halted_state_untouched():
    c = _case(T_HB, False, 2)
    c["ints"][4] = 1
    _, _, prm, status = _both(c)
    assert status == 0
    assert np.all(prm == 0.0)
