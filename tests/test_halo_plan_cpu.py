"""
CPU: how a decomposed block steps beside its halo exchange (csrc/halo_plan.hpp: pcl::OverlapPlan) through its pure-host
trace entry point pcl_halo_plan_trace, against the rule restated here.

The mode is ov = PCL_HALO_OVERLAP (default 1) and dflt = not set; ea = 0, 1 or 2 as pcl_halo_exchange_ahead sets it.  The
facts of a block: active, split2 (classic, 2-D, dimension-split, meqn <= 8), sel0, onek_ok (fused_step_ok), onek_family,
onek_box and x_box (the two interior boxes).

1. What the block offers (pcl_halo_can_overlap): 0 unless active and split2 and ov == 1; else 2 if onek_ok and onek_box;
   else 1 if not (onek_family and dflt) and x_box; else 0.
2. The step's plan (pcl_bc_step): considered only if active and split2 and ov != 0 and sel0.  onek = onek_ok and ea != 1;
   if onek and onek_box: overlapped, one kernel.  Else onek = false and overlapped iff (not (onek_family and dflt) or
   ea == 1) and x_box.  Not overlapped drops every mark.
3. The order of an overlapped step, the first that holds, with have = ea != 0 and filled(q): rim first: onek and ov == 1
   and ea != 0 and have; exchange in front: onek and ov == 1 and ea == 0; test order: ov == 2; else interior first.  The
   new state's exchange is sent ahead behind the step iff ea != 0 and ov == 1.
4. The unsplit step overlaps iff active and ov != 0 and not dflt; a SharpClaw stage iff active and ov != 0 and ndim == 2;
   framed_x_pass runs sequentially iff not overlapping or ov == 2.
5. The marks: two slots, the newest first.  Marking a held buffer is a no-op, marking another moves slot 0 to slot 1 (what
   was there is forgotten); a write empties the slots that hold the buffer; a null buffer is never filled; setting ea,
   a touch and a failure empty both.
"""
import itertools
import os
import re

import numpy as np

from pyclaw_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pyclaw_amd", "csrc", "pclaw.hip")
HDR = os.path.join(ROOT, "pyclaw_amd", "csrc", "halo_plan.hpp")

(CONFIGURE, SET_EA, OFFERS, PLAN, FILLED, EXCHANGED, WRITTEN, TOUCHED, FAILED, UNSPLIT, SHARP, FRAME_SEQ) = range(12)
NOT_OVERLAPPED, RIM_FIRST, EXCHANGE_IN_FRONT, TEST_ORDER, INTERIOR_FIRST = range(5)
ONEK, HAVE, SEND_AHEAD = 8, 16, 32
ACTIVE, SPLIT2, SEL0, ONEK_OK, ONEK_FAMILY, ONEK_BOX, X_BOX = (1 << k for k in range(7))
ALL = 127
MODES = [(0, 1), (1, 1), (2, 1), (3, 1), (1, 0)]          # (ov, set): 0..3 set, and the default


def trace(events):
    """events: (event, a, b) each; returns out[]"""
    n = len(events)
    ev, a, b = (np.array([e[k] for e in events], dtype=np.int32) for k in range(3))
    out = np.full(n, -99, dtype=np.int32)
    L.check(L.lib().pcl_halo_plan_trace(n, L.i(ev), L.i(a), L.i(b), L.i(out)))
    return out.tolist()


class Rule:
    """the rule of the module docstring"""

    def __init__(self):
        self.ov, self.dflt, self.ea, self.mark = 1, True, 0, [0, 0]

    def configure(self, ov, is_set):
        self.ov, self.dflt = ov, not is_set

    def set_ea(self, on):
        self.ea = 2 if on == 2 else 1 if on else 0
        self.mark = [0, 0]

    def offers(self, f):
        if not (f & ACTIVE and f & SPLIT2 and self.ov == 1):
            return 0
        if f & ONEK_OK and f & ONEK_BOX:
            return 2
        if not (f & ONEK_FAMILY and self.dflt) and f & X_BOX:
            return 1
        return 0

    def plan(self, f, q):
        overlapped = onek = False
        if f & ACTIVE and f & SPLIT2 and self.ov != 0 and f & SEL0:
            onek = bool(f & ONEK_OK) and self.ea != 1
            if onek and f & ONEK_BOX:
                overlapped = True
            else:
                onek = False
                overlapped = bool((not (f & ONEK_FAMILY and self.dflt) or self.ea == 1) and f & X_BOX)
        if not overlapped:
            self.mark = [0, 0]
            return NOT_OVERLAPPED
        have = self.ea != 0 and self.filled(q)
        if onek and self.ov == 1 and self.ea != 0 and have:
            order = RIM_FIRST
        elif onek and self.ov == 1 and self.ea == 0:
            order = EXCHANGE_IN_FRONT
        elif self.ov == 2:
            order = TEST_ORDER
        else:
            order = INTERIOR_FIRST
        return order | (ONEK if onek else 0) | (HAVE if have else 0) | (SEND_AHEAD if self.ea != 0 and self.ov == 1 else 0)

    def filled(self, buf):
        return buf != 0 and buf in self.mark

    def exchanged(self, buf):
        if not self.filled(buf):
            self.mark = [buf, self.mark[0]]

    def written(self, buf):
        self.mark = [0 if m == buf else m for m in self.mark]

    def touched(self):
        self.mark = [0, 0]


def by_rule(events):
    r, out = Rule(), []
    for ev, a, b in events:
        res = 0
        if ev == CONFIGURE:
            r.configure(a, b)
        elif ev == SET_EA:
            r.set_ea(a)
        elif ev == OFFERS:
            res = r.offers(a)
        elif ev == PLAN:
            res = r.plan(a, b)
        elif ev == FILLED:
            res = int(r.filled(a))
        elif ev == EXCHANGED:
            r.exchanged(a)
        elif ev == WRITTEN:
            r.written(a)
        elif ev in (TOUCHED, FAILED):
            r.touched()
        elif ev == UNSPLIT:
            res = int(bool(a) and r.ov != 0 and not r.dflt)
        elif ev == SHARP:
            res = int(bool(a) and r.ov != 0 and b == 2)
        elif ev == FRAME_SEQ:
            res = int(not a or r.ov == 2)
        out.append(res)
    return out


def test_every_combination_against_the_rule():
    """all 128 fact sets x the five modes x ea 0..2 x q marked or not: what the block offers, the plan with its order,
    and whether the marks survived it"""
    ev, cases = [], 0
    for (ov, is_set), ea, f, marked in itertools.product(MODES, (0, 1, 2), range(128), (0, 1)):
        ev += [(CONFIGURE, ov, is_set), (SET_EA, ea, 0)]
        if marked:
            ev += [(EXCHANGED, 1, 0), (EXCHANGED, 2, 0)]
        ev += [(OFFERS, f, 0), (FILLED, 1, 0), (PLAN, f, 1), (FILLED, 1, 0), (FILLED, 2, 0)]
        cases += 1
    assert cases == 5 * 3 * 128 * 2
    out = trace(ev)
    assert out == by_rule(ev)
    # every order and every offer occurs, so the comparison is not one of zeros
    plans = [o for e, o in zip(ev, out) if e[0] == PLAN]
    assert {p & 7 for p in plans} == {0, 1, 2, 3, 4} and {o for e, o in zip(ev, out) if e[0] == OFFERS} == {0, 1, 2}


def test_the_three_predicates():
    ev = []
    for ov, is_set in MODES:
        ev += [(CONFIGURE, ov, is_set)]
        ev += [(UNSPLIT, a, 0) for a in (0, 1)]
        ev += [(SHARP, a, nd) for a in (0, 1) for nd in (1, 2, 3)]
        ev += [(FRAME_SEQ, a, 0) for a in (0, 1)]
    out = trace(ev)
    assert out == by_rule(ev)
    per = [out[k + 1:k + 11] for k in range(0, len(out), 11)]
    #           unsplit  sharp (inactive x 3, active x 3)  sequential
    assert per[0] == [0, 0, 0, 0, 0, 0, 0, 0, 1, 0]       # 0: nothing overlaps
    assert per[1] == [0, 1, 0, 0, 0, 0, 1, 0, 1, 0]       # 1, set
    assert per[2] == [0, 1, 0, 0, 0, 0, 1, 0, 1, 1]       # 2: the test order runs on one stream
    assert per[3] == [0, 1, 0, 0, 0, 0, 1, 0, 1, 0]       # any other value: as 1
    assert per[4] == [0, 0, 0, 0, 0, 0, 1, 0, 1, 0]       # the default: the unsplit step exchanges in front


def test_pinned_answers():
    """a few answers spelt out, so that rule and library cannot drift together"""
    thin = ALL & ~ONEK_BOX                                  # no interior box of one-kernel tiles
    aux = ALL & ~(ONEK_OK | ONEK_FAMILY)                    # a solver with aux arrays: never the one-kernel step, decomposed

    def ask(ov, is_set, ea, f, marked=False):
        ev = [(CONFIGURE, ov, is_set), (SET_EA, ea, 0)] + ([(EXCHANGED, 1, 0)] if marked else []) + [(OFFERS, f, 0), (PLAN, f, 1)]
        return tuple(trace(ev)[-2:])

    assert ask(1, 1, 0, ALL) == (2, EXCHANGE_IN_FRONT | ONEK)
    assert ask(1, 0, 0, ALL) == (2, EXCHANGE_IN_FRONT | ONEK)
    assert ask(1, 1, 2, ALL) == (2, INTERIOR_FIRST | ONEK | SEND_AHEAD)             # the first step: nothing sent ahead yet
    assert ask(1, 1, 2, ALL, marked=True) == (2, RIM_FIRST | ONEK | HAVE | SEND_AHEAD)
    assert ask(1, 1, 1, ALL, marked=True) == (2, INTERIOR_FIRST | HAVE | SEND_AHEAD)   # the two-pass order, agreed by the ranks
    assert ask(1, 1, 0, ALL, marked=True) == (2, EXCHANGE_IN_FRONT | ONEK)          # without exchange-ahead a mark is not read
    assert ask(2, 1, 0, ALL) == (0, TEST_ORDER | ONEK)                              # offers nothing, overlaps in the test order
    assert ask(2, 1, 2, ALL, marked=True) == (0, TEST_ORDER | ONEK | HAVE)          # ... and sends nothing ahead
    assert ask(3, 1, 0, ALL) == (0, INTERIOR_FIRST | ONEK)
    assert ask(0, 1, 0, ALL) == (0, NOT_OVERLAPPED)
    # a thin block of the one-kernel family: the exchange in front by default, the two-pass overlap on request or by agreement
    assert ask(1, 0, 0, thin) == (0, NOT_OVERLAPPED)
    assert ask(1, 1, 0, thin) == (1, INTERIOR_FIRST)
    assert ask(1, 0, 1, thin) == (0, INTERIOR_FIRST | SEND_AHEAD)
    assert ask(1, 0, 0, aux) == (1, INTERIOR_FIRST)
    assert ask(1, 0, 0, ALL & ~X_BOX & ~ONEK_BOX) == (0, NOT_OVERLAPPED)
    # the register the calls act on is no property of the block: offered, not planned
    assert ask(1, 1, 0, ALL & ~SEL0) == (2, NOT_OVERLAPPED)
    assert ask(1, 1, 0, ALL & ~ACTIVE) == (0, NOT_OVERLAPPED) and ask(1, 1, 0, ALL & ~SPLIT2) == (0, NOT_OVERLAPPED)


def test_mark_sequences():
    def filled(*ids):
        return [(FILLED, k, 0) for k in ids]

    a, b, c = 1, 2, 3
    ev = filled(a, 0)                                                   # nothing is filled at first, null never
    ev += [(EXCHANGED, a, 0), (EXCHANGED, b, 0)] + filled(a, b, c)
    ev += [(EXCHANGED, c, 0)] + filled(a, b, c)                         # a third: the oldest is forgotten
    ev += [(EXCHANGED, b, 0), (EXCHANGED, a, 0)] + filled(a, b, c)      # a held one: no-op, b stays the older -> a pushes it out
    ev += [(WRITTEN, c, 0)] + filled(a, b, c)                           # drop one
    ev += [(WRITTEN, 7, 0)] + filled(a, b, c)                           # ... that is not held: nothing
    ev += [(EXCHANGED, b, 0), (EXCHANGED, c, 0), (TOUCHED, 0, 0)] + filled(a, b, c)
    ev += [(EXCHANGED, a, 0), (EXCHANGED, b, 0), (FAILED, 0, 0)] + filled(a, b, c)
    ev += [(EXCHANGED, a, 0), (EXCHANGED, b, 0), (SET_EA, 1, 0)] + filled(a, b, c)
    ev += [(EXCHANGED, a, 0), (EXCHANGED, b, 0), (SET_EA, 0, 0)] + filled(a, b, c)
    ev += [(EXCHANGED, a, 0), (EXCHANGED, 0, 0)] + filled(a, 0)         # the null buffer takes a slot and is never filled
    # a slot emptied by a write is not closed up: the next mark still pushes the older slot out
    ev += [(TOUCHED, 0, 0), (EXCHANGED, a, 0), (EXCHANGED, b, 0), (WRITTEN, b, 0), (EXCHANGED, c, 0)] + filled(a, b, c)
    out = trace(ev)
    assert out == by_rule(ev)
    got = [o for e, o in zip(ev, out) if e[0] == FILLED]
    assert got == [0, 0] + [1, 1, 0] + [0, 1, 1] + [1, 0, 1] + [1, 0, 0] + [1, 0, 0] + [0, 0, 0] * 4 + [1, 0] + [0, 0, 1]
    # a not-overlapped plan drops them too, an overlapped one does not
    ev = [(CONFIGURE, 1, 1), (SET_EA, 1, 0), (EXCHANGED, a, 0), (PLAN, ALL, a), (FILLED, a, 0), (PLAN, ALL & ~SEL0, a), (FILLED, a, 0)]
    assert trace(ev)[3:] == [INTERIOR_FIRST | HAVE | SEND_AHEAD, 1, NOT_OVERLAPPED, 0]
    # bad scripts are refused
    lib = L.lib()
    for bad in ((12, 0, 0), (-1, 0, 0), (FILLED, 8, 0), (PLAN, 0, -1)):
        e, x, y = (np.array([v], dtype=np.int32) for v in bad)
        assert lib.pcl_halo_plan_trace(1, L.i(e), L.i(x), L.i(y), L.i(np.zeros(1, dtype=np.int32))) != 0


class Block:
    """The events pcl_bc_step raises on the plan for one overlapped step, in the order pclaw.hip (step_overlapped) raises
    them; q and t2 are buffer ids, swapped by a committed step and swapped back by pcl_undo_step."""

    def __init__(self, facts):
        self.f, self.q, self.t2, self.ev, self.plans = facts, 1, 2, [], []

    def step(self, rule):
        self.plans.append(len(self.ev))
        self.ev.append((PLAN, self.f, self.q))
        p = rule.plan(self.f, self.q)
        order, onek, have = p & 7, bool(p & ONEK), bool(p & HAVE)

        def raise_(e, buf):
            self.ev.append((e, buf, 0))
            (rule.exchanged if e == EXCHANGED else rule.written)(buf)

        if order == NOT_OVERLAPPED:
            self.q, self.t2 = self.t2, self.q
            return
        if onek:
            raise_(WRITTEN, self.t2)
        if order == EXCHANGE_IN_FRONT:
            self.ev.append((TOUCHED, 0, 0))
            rule.touched()
            self.q, self.t2 = self.t2, self.q
            return
        if order == INTERIOR_FIRST and not have:
            raise_(EXCHANGED, self.q)
        if not onek:
            raise_(WRITTEN, self.t2)
        self.q, self.t2 = self.t2, self.q
        if order == RIM_FIRST or p & SEND_AHEAD:
            raise_(EXCHANGED, self.q)

    def undo(self):
        self.q, self.t2 = self.t2, self.q

    def upload(self, rule):
        self.ev.append((TOUCHED, 0, 0))
        rule.touched()


def life(ov, is_set, ea, facts):
    """the sequence of tests/test_gpu_halo.py::test_exchange_ahead_equals_periodic_with_retake: two steps, a rejected one,
    its retake, a step, an upload, two steps -> (the plans, whether the pre-step buffer was still marked at the retake)"""
    rule, blk = Rule(), Block(facts)
    head = [(CONFIGURE, ov, is_set), (SET_EA, ea, 0)]
    rule.configure(ov, is_set)
    rule.set_ea(ea)
    blk.step(rule)
    blk.step(rule)
    blk.step(rule)
    blk.undo()
    at_retake = len(blk.ev)
    blk.ev.append((FILLED, blk.q, 0))
    blk.step(rule)
    blk.step(rule)
    blk.upload(rule)
    blk.step(rule)
    blk.step(rule)
    ev = head + blk.ev
    out = trace(ev)
    assert out == by_rule(ev)
    return [out[2 + k] for k in blk.plans], out[2 + at_retake]


def test_scripted_life_with_retake_and_upload():
    I, R, X, T = INTERIOR_FIRST, RIM_FIRST, EXCHANGE_IN_FRONT, TEST_ORDER
    thin = ALL & ~ONEK_BOX
    # the one-kernel order: the first step and the one behind the upload exchange themselves, every other step finds its
    # frame filled -- the retake too, on the pre-step buffer
    plans, kept = life(1, 1, 2, ALL)
    assert kept == 1
    assert plans == [I | ONEK | SEND_AHEAD] + [R | ONEK | HAVE | SEND_AHEAD] * 4 + [I | ONEK | SEND_AHEAD, R | ONEK | HAVE | SEND_AHEAD]
    # the two-pass order on the same block, and on a thin one
    for f in (ALL, thin):
        plans, kept = life(1, 1, 1, f)
        assert kept == 1
        assert plans == [I | SEND_AHEAD] + [I | HAVE | SEND_AHEAD] * 4 + [I | SEND_AHEAD, I | HAVE | SEND_AHEAD]
    # no exchange-ahead: every step exchanges, whatever is marked (the interior-first order marks the buffer it
    # exchanged, so the pre-step buffer is still marked at the retake; nothing reads it)
    assert life(1, 1, 0, ALL) == ([X | ONEK] * 7, 0)
    assert life(1, 1, 0, thin) == ([I] * 7, 1)
    assert life(1, 0, 0, thin) == ([NOT_OVERLAPPED] * 7, 0)
    # the test order reads no mark to skip an exchange unless exchange-ahead is set, and never sends ahead
    assert life(2, 1, 0, ALL) == ([T | ONEK] * 7, 0)


# ---- the source-level rules ----
def code(path):
    return re.sub(r"//[^\n]*", "", open(path).read())


def body(src, head):
    b = src[src.index(head):]
    return b[:b.index("\n}\n")]


def test_pclaw_names_none_of_the_loose_fields():
    src = code(SRC)
    assert not re.search(r"\b(overlap_dflt|exchange_ahead|ghost_ok|ghosts_\w+|twopass_overlap_ok)\b", src)
    assert not re.search(r"(->|\.)\s*overlap\b", src) and not re.search(r"\b(int|bool)\s+overlap\b", src)
    # one member, its device resources beside it
    solver = body(src, "struct pcl_solver {")
    assert len(re.findall(r"\bOverlapPlan\s+\w+\s*;", src)) == 1 and "pcl::OverlapPlan plan;" in solver
    for name in ("hstream", "ev_h0", "ev_h1", "ev_y"):
        assert re.search(r"\b%s\b" % name, solver), name
    # the environment is read where it was, and handed over
    ready = body(src, "static int comm_ready(pcl_solver *s)")
    assert 'getenv("PCL_HALO_OVERLAP")' in ready and "plan.configure(" in ready and src.count('getenv("PCL_HALO_OVERLAP")') == 1


def test_rule_is_asked_not_restated():
    src = code(SRC)
    # both callers gather the facts and ask the type; the order arrives in step_overlapped as a value
    can = body(src, "int pcl_halo_can_overlap(pcl_solver *s")
    assert "plan.offers(block_facts(s))" in can and "interior_box" not in can and "fused_step_ok" not in can
    step = body(src, "int pcl_bc_step(pcl_solver *s")
    assert "plan.plan(block_facts(s), s->q)" in step and "interior_box" not in step and "fused_step_ok" not in step
    assert step.index("take_valid") < step.index("ahead.matches(") < step.index("ahead_drop") < step.index("plan.plan(") \
        < step.index("step_loading_bcs")
    ovl = body(src, "static int step_overlapped(pcl_solver *s")
    assert "switch (p.order)" in ovl
    for order in ("RIM_FIRST", "EXCHANGE_IN_FRONT", "TEST_ORDER", "INTERIOR_FIRST"):
        assert ovl.count("case OverlapPlan::%s" % order) == 1, order
    # it reads the plan's answer and raises events; it asks no question of its own
    asked = set(re.findall(r"\bplan\.(\w+)\(", ovl))
    assert asked == {"written", "exchanged", "touched", "failed"}, asked
    assert not re.search(r"getenv|\bea\b|\bov\b", ovl)
    # a handle without a communicator leaves block_facts at its first test
    facts = body(src, "OverlapPlan::Facts block_facts(const pcl_solver *s)")
    stmts = [ln.strip() for ln in facts.split("\n")[1:] if ln.strip()]
    assert stmts[1] == "if (!s->halo.active) return f;", stmts[:3]
    # the interior boxes are worked out once, from the geometry alone
    assert src.count("step2ds_interior_box(") == 1 and src.count("x_interior_box(") == 1
    ready = body(src, "static int comm_ready(pcl_solver *s)")
    assert "step2ds_interior_box(" in ready and "x_interior_box(" in ready and "make_args" not in ready


def test_entry_points_that_touch_the_state_say_so():
    src = open(SRC).read()
    touched = []
    for m in re.finditer(r"^int (pcl_\w+)\(pcl_solver \*s\b[^{;]*\{\n([^\n]*)\n([^\n]*)\n", src, re.M):
        if "s->plan.touched();" in m.group(2) or "s->plan.touched();" in m.group(3):
            touched.append(m.group(1))
            assert (m.group(3) if "qt.invalidate" in m.group(2) else m.group(2)).strip().startswith("if (s) s->plan.touched();")
    assert sorted(touched) == sorted([
        "pcl_put_q", "pcl_put_strip", "pcl_bc", "pcl_bc_const", "pcl_sweep", "pcl_step_hyperbolic", "pcl_restore", "pcl_src",
        "pcl_cellfn_apply", "pcl_cellbc_apply", "pcl_select", "pcl_halo_exchange"])


def test_header_is_host_only_with_private_fields():
    raw = open(HDR).read()
    hdr = code(HDR)
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", raw, re.M)
    assert not [i for i in includes if "hip" in i.lower()], includes
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__device__|getenv|chrono|\bclock\b|\btime\s*\(", hdr)
    cls = hdr[hdr.index("class OverlapPlan {"):]
    cls = cls[:cls.index("\n};\n")]
    public, private = cls[:cls.index("private:")], cls[cls.index("private:"):]
    assert "public:" in public and "public:" not in private
    for decl in (r"\bint\s+ov\b", r"\bea\b\s*=\s*0", r"\bbool\s+dflt\b", r"\*\s*mark\s*\[2\]"):
        assert re.search(decl, private) and not re.search(decl, public), decl
    # every field is named in the header comment with the events that change it
    head = raw[:raw.index("#pragma once")]
    for word in ("ov, dflt", "ea ", "mark[2]", "configure()", "set_exchange_ahead()", "exchanged()", "written()", "touched()",
                 "failed()", "plan()"):
        assert word in head, word
