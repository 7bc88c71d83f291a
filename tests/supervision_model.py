"""A pure Python model of one dispatcher of the engine with supervision: DESIGN.md §2 (the BSP superstep,
tests/prio_model.PrioModel) plus §2.5 (Behaviors.supervise(..).onFailure(strategy), the PreRestart and PostStop
signals; the reference: TY/internal/Supervision.scala:43-52,128-160,311-406, pinned by SupervisionSpec.scala:100-245).

  a tick is a superstep with mail; inside the drain of actor a at tick t --
    1. a compiled case may end in FAIL: its actions have run, the message is delivered, failures++, and the
       exception class is the case's `next`;
    2. the entries are those of the kind a was registered with, inner first; the failure goes to the first entry
       whose mask has the class.  None, or STOP: the actor stops.  RESUME: nothing changes, resumes++;
    3. RESTART with count c and deadline d (time is left iff there is no deadline or t <= d): if max_restarts !=
       -1 and c >= max_restarts and time is left, the failure goes on to the next outer entry that catches it;
       else PreRestart runs on the current behaviour, c := time left ? c + 1 : 1, d := (a deadline and time left)
       ? d : t + within, the inner entries' counts and deadlines are cleared, the kind becomes the initial
       kind, the reset words take their values, restarts++, and the drain goes on with the next message;
    4. every stop (a `stopped` result, a failure that stops) runs PostStop on the current behaviour, stops++;
    5. a signal runs the signal cases (first test: payload == the signal) with the actor itself as the sender;
       its actions apply, its tells count as emitted, no matching case is nothing.

It takes the same calls as GpuEngine, so with no failing case it is pinned to the frozen oracle.
"""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, STOPPED, UNHANDLED, PrioModel

FAIL = typed.RES_FAIL
NO_DEADLINE = 0xFFFFFFFF
INFO_KEYS = ("failures", "resumes", "restarts", "stops", "ticks")


class SupervisionModel(PrioModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rows = None        # per compiled behaviour: its entries, inner first
        self.n_levels = 0
        self.init_kind = None   # the kind every actor was registered with
        self.count = None       # [actor][level]
        self.deadline = None    # [actor][level], 0: none
        self.s = dict(failures=0, resumes=0, restarts=0, stops=0)

    # ------------------------------------------------------------ setup
    def register_range(self, first, count, kind, init_state=None):
        super().register_range(first, count, kind, init_state)
        if self.init_kind is not None:
            self.init_kind[first:first + count] = kind

    def set_supervision(self, rows):
        assert self.kmax == 1 and self.c["supersteps"] == 0
        self.rows = [list(r) for r in rows]
        self.n_levels = max([len(r) for r in self.rows] + [1])
        assert 1 <= self.n_levels <= typed.MAX_SUPERVISORS and 1 <= len(self.rows) <= typed.MAX_BEHAVIORS
        self.init_kind = self.kind.copy()
        self.count = np.zeros((self.n, self.n_levels), np.int64)
        self.deadline = np.zeros((self.n, self.n_levels), np.int64)

    # ------------------------------------------------------------ reading
    def supervision_info(self) -> dict:
        return dict(self.s, ticks=self.c["supersteps"])

    def read_supervision(self, a) -> dict:
        o = dict(initial_kind=0, count=np.zeros(4, np.uint32), remaining=np.full(4, NO_DEADLINE, np.uint32))
        if self.rows is None:
            return o
        o["initial_kind"] = int(self.init_kind[a])
        now = self.c["supersteps"]
        for k in range(self.n_levels):
            o["count"][k] = self.count[a, k]
            d = int(self.deadline[a, k])
            o["remaining"][k] = NO_DEADLINE if d == 0 else max(d - now, 0)
        return o

    # ------------------------------------------------------------ behaviours
    def _compiled_s(self, a, w, src, pay, signal):
        """-> (result, exception class)"""
        t = self.tables
        b = int(self.kind[a]) - typed.KIND_COMPILED
        if t is None or b >= t.n_behaviors:
            return UNHANDLED, 0
        for ci in range(int(t.first[b]), int(t.first[b + 1])):
            C = t.cases[ci]
            if bool(C.result & typed.CASE_SIGNAL) != signal:
                continue
            if not self._cmp(C.cmp1, self._operand(C.src1, C.word1, C.k1, pay, w, src, a),
                             self._operand(C.src2, C.word2, C.k2, pay, w, src, a)):
                continue
            if not self._cmp(C.cmp2, self._operand(C.src3, C.word3, C.k3, pay, w, src, a),
                             self._operand(C.src4, C.word4, C.k4, pay, w, src, a)):
                continue
            for i in range(C.act_first, C.act_first + C.act_count):  # in order
                A = t.acts[i]
                v = self._operand(A.src, A.sword, A.k, pay, w, src, a)
                x = A.word & 1
                if A.op == typed.A_SET:
                    w[x] = v
                elif A.op == typed.A_ADD:
                    w[x] = (w[x] + v) & M64
                elif A.op == typed.A_MAX:
                    w[x] = max(w[x], v)
                elif A.op == typed.A_MIN:
                    w[x] = min(w[x], v)
                elif A.op == typed.A_TELL:
                    if A.dsrc == typed.V_SELF:
                        d = (a + A.dk) % self.n
                    else:
                        d = self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a)
                    self._emit(a, min(d, M32), ((v & 0xFFFFFF) | A.or_mask) if A.or_mask else (v & M32))
            res = C.result & ~typed.CASE_SIGNAL
            if res == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME, 0
            return res, C.next
        return UNHANDLED, 0

    def _signal(self, a, w, code):
        if int(self.kind[a]) >= typed.KIND_COMPILED:
            self._compiled_s(a, w, a, code, True)

    def _failed(self, a, w, res, cls, t) -> int:
        """the supervisor's catch clause: SAME (resumed or restarted) or STOPPED (PostStop has run)"""
        if res == FAIL:
            self.s["failures"] += 1
            ik = int(self.init_kind[a])
            b = ik - typed.KIND_COMPILED
            row = self.rows[b] if 0 <= b < len(self.rows) else []
            for lev, E in enumerate(row):  # inner first
                if not (E.class_mask >> (cls & 31)) & 1:
                    continue
                if E.strategy == typed.SUP_RESUME:
                    self.s["resumes"] += 1
                    return SAME
                if E.strategy != typed.SUP_RESTART:
                    break
                c, d = int(self.count[a, lev]), int(self.deadline[a, lev])
                left = d == 0 or t <= d
                if E.max_restarts != -1 and c >= E.max_restarts and left:
                    continue  # rethrown (:316)
                self._signal(a, w, typed.SIGNAL_PRERESTART)
                self.count[a, lev] = c + 1 if left else 1
                self.deadline[a, lev] = d if (d != 0 and left) else t + E.within
                self.count[a, :lev] = 0
                self.deadline[a, :lev] = 0
                self.kind[a] = ik
                for x in range(2):
                    if (E.reset_mask >> x) & 1:
                        w[x] = int(E.reset[x])
                self.s["restarts"] += 1
                return SAME
        self._signal(a, w, typed.SIGNAL_POSTSTOP)
        self.s["stops"] += 1
        return STOPPED

    # ------------------------------------------------------------ supersteps
    def step(self) -> bool:
        if self.rows is None:
            return super().step()
        msgs = self.backlog + self.emitted_q + self.staged_q
        if not msgs:
            return False
        t = self.c["supersteps"] + 1  # this tick
        inbox = {}
        for d, s, p in msgs:
            inbox.setdefault(d, []).append((s, p))
        sizes = np.zeros(self.n, np.int64)
        self.backlog, self._out = [], []
        for a in sorted(inbox):
            q = inbox[a]
            L = len(q)
            sizes[a] = L
            if not self.alive[a]:
                self.c["dead_letters"] += L
                continue
            C, T = self._limits(a)
            keep = L if C == 0 else min(L, C)
            self.c["dead_letters"] += L - keep
            adm = q[:keep]
            nd = min(keep, T)
            w = [int(self.words[a, 0]), int(self.words[a, 1])]
            for i in range(nd):
                sv, pv = adm[i]
                if int(self.kind[a]) >= typed.KIND_COMPILED:
                    r, cls = self._compiled_s(a, w, sv, pv, False)
                else:
                    r, cls = self._apply(a, w, sv, pv), 0
                self.c["delivered"] += 1
                if r == UNHANDLED:
                    self.c["unhandled"] += 1
                if r in (FAIL, STOPPED):
                    r = self._failed(a, w, r, cls, t)
                if r == STOPPED:
                    self.alive[a] = 0
                    self.c["dead_letters"] += nd - i - 1
                    break
            self.words[a, 0], self.words[a, 1] = w[0], w[1]
            self.backlog += [(a, s, p) for s, p in adm[nd:]]
        self.emitted_q, self.staged_q = self._out, []
        self.inbox_sizes.append(sizes)
        self.c["supersteps"] += 1
        return True
