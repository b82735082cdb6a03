"""
CPU: which form of the dimension-split 2-D step runs (csrc/step_form.hpp: pcl::StepForm) through its pure-host trace
entry point pcl_step_form_trace, against the rule of DESIGN.md 4.1a restated here.

With k = (tuned steps so far) mod 256 - 64: at k = 0 the best times reset and the window is gated iff listed >= 0 and
4 listed <= ntiles, a gated window's form being one kernel (1); an ungated window's steps k = 0..3 run one kernel and
k = 4..7 the two passes (0), those with k mod 4 != 0 timed and the best time of each form kept; at k = 8, ungated, the
form becomes the two passes iff t0 < 0.98 t1.  A step that is not tuned takes can ? 1 : 0 and leaves the window alone.
"""
import numpy as np

from pyclaw_amd import _lib as L

NT = 1000
STEP, PLAIN, ADOPTED, RAN, FORGET, COUNT = range(6)


def trace(events, ntiles=NT):
    """events: (event, a, b, listed, seconds) each; returns out[]"""
    n = len(events)
    ev = np.array([e[0] for e in events], dtype=np.int32)
    a = np.array([e[1] for e in events], dtype=np.int32)
    b = np.array([e[2] for e in events], dtype=np.int32)
    listed = np.array([e[3] for e in events], dtype=np.int64)
    sec = np.array([e[4] for e in events], dtype=np.float64)
    out = np.full(n, -99, dtype=np.int32)
    L.check(L.lib().pcl_step_form_trace(n, L.i(ev), L.i(a), L.i(b), listed.ctypes.data_as(L.C.POINTER(L.C.c_long)), ntiles,
                                        L.d(sec), L.i(out)))
    return out.tolist()


def step(can=1, tune=1, listed=-1, seconds=1.0):
    return (STEP, can, tune, listed, seconds)


class Rule:
    """the rule of the module docstring"""

    def __init__(self):
        self.now, self.n, self.t, self.gated = 1, 0, [0.0, 0.0], False

    def step(self, can, tune, listed, ntiles, seconds):
        """-> (form, timed)"""
        if not tune:
            return (1 if can else 0), False
        k = self.n % 256 - 64
        timed = False
        if k == 0:
            self.t = [1e30, 1e30]
            self.gated = listed >= 0 and 4 * listed <= ntiles
            if self.gated:
                self.now = 1
        if not self.gated and 0 <= k <= 7:
            form = 1 if k <= 3 else 0
            timed = k % 4 != 0
            if timed:
                self.t[form] = min(self.t[form], seconds)
        else:
            if not self.gated and k == 8:
                self.now = 0 if self.t[0] < 0.98 * self.t[1] else 1
            form = self.now
        self.n += 1
        return form, timed

    def plain_onek(self, can, mode):
        if not can:
            return False
        if mode != 2:
            return True
        k = self.n % 256 - 64
        if k == 0 or (not self.gated and 0 <= k <= 8):
            return False
        return self.now == 1

    def adopted(self, mode):
        if mode == 2:
            self.n += 1


def by_rule(events, ntiles=NT):
    r, out = Rule(), []
    for ev, a, b, listed, sec in events:
        if ev == STEP:
            form, timed = r.step(a, b, listed, ntiles, sec)
            out.append(form | (2 if timed else 0))
        elif ev == PLAIN:
            out.append(int(r.plain_onek(a, b)))
        elif ev == ADOPTED:
            r.adopted(b)
            out.append(1)
    return out


def forms(out):
    return [o & 1 for o in out]


def window_times(n, t_onek, t_twopass, first=0):
    """n tuned steps from tuned step `first` on; a trial step takes its form's time (every other step's is not read)"""
    ev = []
    for i in range(first, first + n):
        k = i % 256 - 64
        ev.append(step(seconds=t_twopass if 4 <= k <= 7 else t_onek))
    return ev


def test_600_tuned_steps_two_passes_faster_then_within_two_percent():
    # two passes 10 % faster: they take over behind the trials, and the second window's trials run one kernel again
    ev = window_times(600, 1.0, 0.9)
    out = trace(ev)
    want = [1] * 68 + [0] * (320 - 68) + [1] * 4 + [0] * (576 - 324) + [1] * 4 + [0] * (600 - 580) 
    assert forms(out) == want
    timed = [i for i, o in enumerate(out) if o & 2]
    assert timed == [65, 66, 67, 69, 70, 71, 321, 322, 323, 325, 326, 327, 577, 578, 579, 581, 582, 583]
    assert out == by_rule(ev)
    # within 2 %: one kernel stays (the two passes must win by more than that)
    for t0 in (0.99, 0.9801, 1.0, 1.5):
        ev = window_times(600, 1.0, t0)
        out = trace(ev)
        assert forms(out) == [1] * 68 + [0] * 4 + [1] * (324 - 72) + [0] * 4 + [1] * (580 - 328) + [0] * 4 + [1] * 16, t0
        assert out == by_rule(ev)
    # the bound itself: strictly below 0.98 t1
    assert forms(trace(window_times(80, 1.0, 0.98)))[72:] == [int(not 0.98 < 0.98 * 1.0)] * 8
    assert forms(trace(window_times(80, 1.0, 0.9799)))[72:] == [0] * 8
    # the verdict takes the BEST time of each form
    ev = window_times(80, 1.0, 0.99)
    ev[70] = step(seconds=0.5)
    assert forms(trace(ev))[72:] == [0] * 8
    ev[66] = step(seconds=0.5)
    assert forms(trace(ev))[72:] == [1] * 8


def test_first_trial_step_of_a_form_is_untimed():
    for odd in (1e9, 1e40, 1e-9):
        # on the first two-pass trial step (k = 4): counted, a tiny time would hand the window to the two passes
        ev = window_times(100, 1.0, 0.99)
        ev[68] = step(seconds=odd)
        out = trace(ev)
        assert not out[68] & 2 and forms(out)[72:] == [1] * 28, odd
        # on the first one-kernel trial step (k = 0): counted, a tiny time would keep one kernel against 10 %
        ev = window_times(100, 1.0, 0.9)
        ev[64] = step(seconds=odd)
        out = trace(ev)
        assert not out[64] & 2 and forms(out)[72:] == [0] * 28, odd
        assert out == by_rule(ev)


def test_gate():
    def run(listed_at_gate, ntiles, elsewhere=-1):
        ev = window_times(100, 1.0, 0.5)
        ev = [(e[0], e[1], e[2], elsewhere, e[4]) for e in ev]
        ev[64] = step(listed=listed_at_gate, seconds=1.0)
        out = trace(ev, ntiles)
        assert out == by_rule(ev, ntiles)
        return out

    gated, trials = [1] * 100, [1] * 68 + [0] * 32
    assert run(250, 1000) == gated                      # 4 listed == ntiles: no trial, nothing timed
    assert run(0, 1000) == gated
    assert forms(run(250, 999)) == trials               # 4 listed == ntiles + 1
    assert forms(run(251, 1000)) == trials
    assert forms(run(-1, 1000)) == trials               # no current count
    assert forms(run(-1, 1000, elsewhere=0)) == trials  # the count is read at the gate step only
    assert run(250, 1000, elsewhere=1000) == gated
    # a gated window behind a window that chose the two passes returns to one kernel
    ev = window_times(600, 1.0, 0.9)
    ev[320] = step(listed=10)
    out = trace(ev)
    assert out[:576] == [1] * 64 + [1, 3, 3, 3, 0, 2, 2, 2] + [0] * (320 - 72) + [1] * (576 - 320)
    assert out == by_rule(ev)


def test_untuned_steps_do_not_advance_the_window():
    # two untuned steps (can: one kernel; cannot: two passes) behind every tuned one
    ev, tuned_at = [], []
    for i in range(100):
        k = i - 64
        tuned_at.append(len(ev))
        ev += [step(seconds=0.5 if 4 <= k <= 7 else 1.0), step(can=1, tune=0, listed=0, seconds=1e-9),
               step(can=0, tune=0, listed=0, seconds=1e-9)]
    out = trace(ev)
    assert out == by_rule(ev)
    assert [out[j] for j in tuned_at] == [1] * 64 + [1, 3, 3, 3, 0, 2, 2, 2] + [0] * 28
    assert all(out[j + 1] == 1 and out[j + 2] == 0 for j in tuned_at)


def test_cannot_gives_two_passes_throughout():
    ev = [step(can=0, tune=0, listed=0, seconds=1e-9) for _ in range(600)]
    out = trace(ev)
    assert out == [0] * 600 and out == by_rule(ev)
    # counted all the same, and last() follows
    assert trace(ev[:5] + [(COUNT, 0, 0, 0, 0.0), (COUNT, 1, 0, 0, 0.0), (FORGET, 0, 0, 0, 0.0)])[5:] == [5, 0, -1]


def test_next_is_plain_onek_at_every_phase():
    for listed, t_two in ((-1, 0.5), (-1, 1.0), (10, 0.5)):     # trials: two passes win / one kernel stays; gated
        ev = []
        for e in window_times(600, 1.0, t_two):
            i = len(ev) // 5
            if i % 256 == 64:
                e = step(listed=listed, seconds=e[4])
            ev += [(PLAIN, 1, 2, 0, 0.0), (PLAIN, 1, 1, 0, 0.0), (PLAIN, 1, 0, 0, 0.0), (PLAIN, 0, 2, 0, 0.0), e]
        out = trace(ev)
        assert out == by_rule(ev)
        plain = out[0::5]
        if listed >= 0:
            want = [int(i % 256 != 64) for i in range(600)]
        else:
            won = t_two < 0.98
            want = [int(not 64 <= i % 256 <= 72 and not (won and i > 72)) for i in range(600)]
        assert plain == want
        assert out[1::5] == [1] * 600 and out[2::5] == [1] * 600 and out[3::5] == [0] * 600


def test_adopted_advances_the_window_in_mode_2_only():
    tail = window_times(80, 1.0, 0.5)
    for mode, first in ((2, 64), (1, 0), (0, 0)):
        ev = [(ADOPTED, 0, mode, 0, 0.0)] * 64 + window_times(80, 1.0, 0.5, first=first)
        out = trace(ev)
        assert out[:64] == [1] * 64                         # last() is the one-kernel form
        assert out == by_rule(ev)
        want = [1, 3, 3, 3, 0, 2, 2, 2] + [0] * 72 if mode == 2 else [1] * 64 + [1, 3, 3, 3, 0, 2, 2, 2] + [0] * 8
        assert out[64:] == want, mode
    # an adopted step counts as a one-kernel step; ran() counts and leaves last() alone
    ev = tail[:3] + [(ADOPTED, 0, 2, 0, 0.0), (FORGET, 0, 0, 0, 0.0), (RAN, 0, 0, 0, 0.0), (RAN, 1, 0, 0, 0.0),
                     (COUNT, 1, 0, 0, 0.0), (COUNT, 0, 0, 0, 0.0)]
    assert trace(ev)[3:] == [1, -1, -1, -1, 5, 1]
