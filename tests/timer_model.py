"""A pure Python model of one dispatcher of the engine with timers: DESIGN.md §2 (the BSP superstep,
tests/prio_model.PrioModel) plus §2.3 (Behaviors.withTimers / TimerScheduler in logical time; the reference:
TY/internal/TimerSchedulerImpl.scala:61-172, pinned by TimerSpec.scala:45-314).

  one superstep is one tick; tick s, per actor --
    1. inbox = backlog ++ arrivals emitted in s-1 (canonical order) ++ host-staged tells ++ the tick's
       TimerMsgs in key order (every alive actor's active slot whose next fire is s; a periodic slot's next
       fire becomes s + period, a single slot's "none to come");
    2. admission by position, drain of the first min(len, T) -- unchanged (a TimerMsg over capacity is a
       dead letter);
    3. a drained message with tag 0xFF is a TimerMsg (interceptTimerMsg): it counts as delivered; slot
       inactive or another generation (mod 2^22) -> discarded, else a single slot becomes inactive and the
       behaviour runs on the slot's stored payload with sender = self;
    4. a stop makes every slot of the actor inactive.
  A run ends when no mail is in flight and no timer is pending (active with a fire still to come); a tick
  without mail is still a superstep of the budget and counts in `ticks`, not in `supersteps`.

It takes the same calls as GpuEngine, so with no timer in use it is pinned to the frozen oracle.
"""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, STOPPED, UNHANDLED, PrioModel

NONE = 0xFFFFFFFF
TAG_TIMER = 0xFF
GEN_MASK = (1 << 22) - 1
MAX_DELAY = (1 << 31) - 1


class Slot:
    __slots__ = ("active", "next", "period", "gen", "payload")

    def __init__(self):
        self.active, self.next, self.period, self.gen, self.payload = False, NONE, 0, 0, 0


def clamp_delay(d: int) -> int:
    """a computed delay is a wrapped 64-bit sum read as signed: below 1 counts as 1, above 2^31 - 1 is clamped"""
    d &= M64
    if d >= 1 << 63 or d < 1:
        return 1
    return min(d, MAX_DELAY)


class TimerModel(PrioModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n_keys = 0
        self.slots = None       # [actor][key]
        self.agen = None        # the actor's generation counter (timerGen): the next generation to hand out
        self.now = 0            # ticks run so far
        self.t = dict(fired=0, discarded=0, ticks=0)

    # ------------------------------------------------------------ setup
    def set_timers(self, n_keys: int):
        assert 1 <= n_keys <= 4 and self.kmax == 1
        self.n_keys = n_keys
        self.slots = [[Slot() for _ in range(n_keys)] for _ in range(self.n)]
        self.agen = [1] * self.n

    def _start(self, a, key, periodic, delay, payload, period=None):
        s = self.slots[a][key]
        s.active = True
        s.gen = self.agen[a]
        self.agen[a] += 1
        s.next = self.now + delay
        s.period = (delay if period is None else period) if periodic else 0
        s.payload = payload & M32

    def _cancel(self, a, key):
        s = self.slots[a][key]
        s.active, s.next, s.period = False, NONE, 0

    def start_timers(self, first, count, key, delay=1, *, periodic=False, delays=None, payload=0):
        assert self.n_keys and key < self.n_keys
        for i in range(count):
            a = first + i
            if not self.alive[a]:
                continue
            d = int(delays[i]) if delays is not None else int(delay)
            # (the first fire after delays[i]; a periodic timer's period is `delay`)
            self._start(a, key, periodic, min(max(d, 1), MAX_DELAY), payload, min(max(int(delay), 1), MAX_DELAY))

    def tell(self, dst, payload, src=None):
        if self.n_keys:
            assert not np.any((np.atleast_1d(np.asarray(payload, np.uint32)) >> 24) == TAG_TIMER), "tag 0xFF is reserved"
        super().tell(dst, payload, src)

    # ------------------------------------------------------------ reading
    def timer_info(self) -> dict:
        act = pend = 0
        if self.slots:
            for row in self.slots:
                for s in row:
                    act += s.active
                    pend += s.active and s.next != NONE
        return dict(fired=self.t["fired"], discarded=self.t["discarded"], active=int(act), pending=int(pend),
                    ticks=self.t["ticks"])

    def read_timers(self, a) -> dict:
        o = dict(active=np.zeros(4, np.uint32), remaining=np.full(4, NONE, np.uint32), period=np.zeros(4, np.uint32),
                 payload=np.zeros(4, np.uint32), generation=np.zeros(4, np.uint32))
        for k in range(self.n_keys):
            s = self.slots[a][k]
            o["active"][k] = s.active
            o["remaining"][k] = NONE if s.next == NONE else s.next - self.now
            o["period"][k] = s.period
            o["payload"][k] = s.payload
            o["generation"][k] = s.gen & M32
        return o

    # ------------------------------------------------------------ behaviours
    def _operand(self, src, word, k, pay, w, sender, self_id):
        if src == typed.V_TIMER:
            on = self.n_keys and word < self.n_keys and self.slots[self_id][word].active
            return ((1 if on else 0) + k) & M64
        return super()._operand(src, word, k, pay, w, sender, self_id)

    def _compiled(self, a, w, src, pay):
        t = self.tables
        b = int(self.kind[a]) - typed.KIND_COMPILED
        if t is None or b >= t.n_behaviors:
            return UNHANDLED
        for ci in range(int(t.first[b]), int(t.first[b + 1])):
            C = t.cases[ci]
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
                elif A.op in (typed.A_TIMER_SINGLE, typed.A_TIMER_PERIODIC):
                    d = clamp_delay(self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a))
                    self._cancel(a, A.word)
                    self._start(a, A.word, A.op == typed.A_TIMER_PERIODIC, d,
                                ((v & 0xFFFFFF) | A.or_mask) if A.or_mask else (v & M32))
                elif A.op == typed.A_TIMER_CANCEL:
                    self._cancel(a, A.word)
                elif A.op == typed.A_TIMER_CANCEL_ALL:
                    for k in range(self.n_keys):
                        self._cancel(a, k)
            if C.result == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME
            return C.result
        return UNHANDLED

    # ------------------------------------------------------------ supersteps
    def _pending(self) -> bool:
        return bool(self.slots) and any(s.active and s.next != NONE for row in self.slots for s in row)

    def step(self) -> bool:
        if not self.n_keys:
            return super().step()
        if not (self.backlog or self.emitted_q or self.staged_q or self._pending()):
            return False
        self.now += 1
        self.t["ticks"] += 1
        fires = []
        for a in range(self.n):
            if not self.alive[a]:
                continue
            for k, s in enumerate(self.slots[a]):
                if s.active and s.next == self.now:
                    fires.append((a, a, (TAG_TIMER << 24) | (k << 22) | (s.gen & GEN_MASK)))
                    s.next = self.now + s.period if s.period else NONE
        self.t["fired"] += len(fires)
        msgs = self.backlog + self.emitted_q + self.staged_q + fires
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
                self.c["delivered"] += 1
                if pv >> 24 == TAG_TIMER:  # interceptTimerMsg
                    key = (pv >> 22) & 3
                    s = self.slots[a][key] if key < self.n_keys else None
                    if s is None or not s.active or (s.gen ^ pv) & GEN_MASK:
                        self.t["discarded"] += 1
                        continue
                    if not s.period:
                        s.active = False
                    sv, pv = a, s.payload
                r = self._apply(a, w, sv, pv)
                if r == UNHANDLED:
                    self.c["unhandled"] += 1
                if r == STOPPED:
                    self.alive[a] = 0
                    self.c["dead_letters"] += nd - i - 1
                    for k in range(self.n_keys):
                        self._cancel(a, k)
                    break
            self.words[a, 0], self.words[a, 1] = w[0], w[1]
            self.backlog += [(a, s, p) for s, p in adm[nd:]]
        self.emitted_q, self.staged_q = self._out, []
        self.inbox_sizes.append(sizes)
        if msgs:
            self.c["supersteps"] += 1
        return True
