"""A pure Python model of one dispatcher of the engine with receive timeouts: the timers' model
(tests/timer_model.TimerModel) plus §2.7 (context.setReceiveTimeout in logical time; the reference:
akka-actor dungeon/ReceiveTimeout.scala:18-74, typed ActorContextAdapter.scala:120-131, pinned by
ReceiveTimeoutSpec.scala:63-278 and ActorContextSpec.scala:565-610).

  every actor has a delay (0: no timeout set), a message and a next fire (a tick, or none to come); tick s --
    1. the inbox of §2.3, then per actor one more item after the tick's TimerMsgs: the receive-timeout envelope
       (tag 0xFB, sender = the actor) of every alive actor with a timeout set and next fire s; the next fire
       becomes "none to come";
    2. admission and drain unchanged; a drained envelope counts as delivered; with no timeout set at that point of
       the window it is discarded, else the behaviour runs on the message stored now with sender = self;
    3. a case may set (d, msg): next fire s + d, or cancel: delay 0, none to come -- whatever the message;
    4. after its case a message whose tag (of the payload the behaviour saw) is not transparent, and the envelope's
       message always, moves the next fire to s + delay if a timeout is set; discarded TimerMsgs and envelopes,
       queued messages and dead letters do not;
    5. any stop turns the timeout off.
  A pending receive timeout (set, with a fire to come) keeps the run going exactly as a pending timer does.

With no timeout set it is TimerModel, and through it pinned to the frozen oracle.
"""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, STOPPED, UNHANDLED
from tests.timer_model import GEN_MASK, MAX_DELAY, NONE, TAG_TIMER, TimerModel, clamp_delay

TAG_RT = 0xFB


class ReceiveTimeoutModel(TimerModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rt_on = False
        self.transparent = frozenset()
        self.rt_delay = self.rt_pay = self.rt_next = None
        self.rt = dict(fired=0, discarded=0)
        self._cur = None  # the timeout of the actor whose case runs: [delay, payload, changed]

    # ------------------------------------------------------------ setup
    def set_receive_timeout(self, transparent_tags=()):
        assert self.n_keys and not self.rt_on, "on top of the timers, once"
        self.rt_on = True
        self.transparent = frozenset(int(t) for t in transparent_tags)
        self.rt_delay, self.rt_pay, self.rt_next = [0] * self.n, [0] * self.n, [NONE] * self.n

    def start_receive_timeout(self, first, count, delay, payload=0):
        assert self.rt_on
        d = min(int(delay), MAX_DELAY)
        for a in range(first, first + count):
            if not self.alive[a]:
                continue
            self.rt_delay[a] = d
            self.rt_next[a] = self.now + d if d else NONE
            if d:
                self.rt_pay[a] = payload & M32

    def tell(self, dst, payload, src=None):
        if self.rt_on:
            assert not np.any((np.atleast_1d(np.asarray(payload, np.uint32)) >> 24) == TAG_RT), "tag 0xFB is reserved"
        super().tell(dst, payload, src)

    def start_timers(self, first, count, key, delay=1, *, periodic=False, delays=None, payload=0):
        assert not (self.rt_on and (payload & M32) >> 24 == TAG_RT), "tag 0xFB is reserved"
        super().start_timers(first, count, key, delay, periodic=periodic, delays=delays, payload=payload)

    # ------------------------------------------------------------ reading
    def receive_timeout_info(self) -> dict:
        ns = npd = 0
        if self.rt_on:
            for a in range(self.n):
                if self.rt_delay[a]:
                    ns += 1
                    npd += self.rt_next[a] != NONE
        return dict(fired=self.rt["fired"], discarded=self.rt["discarded"], set=ns, pending=npd)

    def read_receive_timeout(self, first=0, count=None) -> dict:
        count = self.n - first if count is None else count
        o = dict(delay=np.zeros(count, np.uint32), remaining=np.full(count, NONE, np.uint32), payload=np.zeros(count, np.uint32))
        if self.rt_on:
            for i in range(count):
                a = first + i
                o["delay"][i] = self.rt_delay[a]
                o["remaining"][i] = NONE if self.rt_next[a] == NONE else self.rt_next[a] - self.now
                o["payload"][i] = self.rt_pay[a]
        return o

    # ------------------------------------------------------------ behaviours
    def _compiled(self, a, w, src, pay):
        if not self.rt_on:
            return super()._compiled(a, w, src, pay)
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
                msg = ((v & 0xFFFFFF) | A.or_mask) if A.or_mask else (v & M32)
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
                    self._emit(a, min(d, M32), msg)
                elif A.op in (typed.A_TIMER_SINGLE, typed.A_TIMER_PERIODIC):
                    d = clamp_delay(self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a))
                    self._cancel(a, A.word)
                    self._start(a, A.word, A.op == typed.A_TIMER_PERIODIC, d, msg)
                elif A.op == typed.A_TIMER_CANCEL:
                    self._cancel(a, A.word)
                elif A.op == typed.A_TIMER_CANCEL_ALL:
                    for k in range(self.n_keys):
                        self._cancel(a, k)
                elif A.op == typed.A_SET_RECEIVE_TIMEOUT:
                    self._cur[0] = clamp_delay(self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a))
                    self._cur[1] = msg
                    self._cur[2] = True
                elif A.op == typed.A_CANCEL_RECEIVE_TIMEOUT:
                    self._cur[0] = 0
                    self._cur[2] = True
            if C.result == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME
            return C.result
        return UNHANDLED

    # ------------------------------------------------------------ supersteps
    def _pending(self) -> bool:
        if super()._pending():
            return True
        return self.rt_on and any(self.alive[a] and self.rt_delay[a] and self.rt_next[a] != NONE for a in range(self.n))

    def step(self) -> bool:
        if not self.rt_on:
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
                    self.t["fired"] += 1
            if self.rt_delay[a] and self.rt_next[a] == self.now:  # one more key after the last
                fires.append((a, a, TAG_RT << 24))
                self.rt_next[a] = NONE
                self.rt["fired"] += 1
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
                envelope = False
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
                elif pv >> 24 == TAG_RT:
                    if not self.rt_delay[a]:
                        self.rt["discarded"] += 1
                        continue
                    envelope = True
                    sv, pv = a, self.rt_pay[a]
                self._cur = [self.rt_delay[a], self.rt_pay[a], False]
                r = self._apply(a, w, sv, pv)
                delay, pay, changed = self._cur
                if changed:
                    self.rt_delay[a] = delay
                    if delay:
                        self.rt_pay[a] = pay
                if r == UNHANDLED:
                    self.c["unhandled"] += 1
                if r == STOPPED:
                    self.alive[a] = 0
                    self.c["dead_letters"] += nd - i - 1
                    for k in range(self.n_keys):
                        self._cancel(a, k)
                    self.rt_delay[a], self.rt_next[a] = 0, NONE
                    break
                if changed or (self.rt_delay[a] and (envelope or (pv >> 24) not in self.transparent)):
                    self.rt_next[a] = self.now + self.rt_delay[a] if self.rt_delay[a] else NONE
            self.words[a, 0], self.words[a, 1] = w[0], w[1]
            self.backlog += [(a, s, p) for s, p in adm[nd:]]
        self.emitted_q, self.staged_q = self._out, []
        self.inbox_sizes.append(sizes)
        if msgs:
            self.c["supersteps"] += 1
        return True
