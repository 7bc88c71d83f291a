"""A pure Python model of one dispatcher of the engine with sharded entities: the receive timeouts' model
(tests/receive_timeout_model.ReceiveTimeoutModel) plus §2.13 (start on demand, Passivate, buffered
restart; the reference: akka-cluster-sharding Shard.scala getOrCreateEntity :504-516, passivate :405-417,
deliverMessage / appendToMessageBuffer :469-496, entityTerminated / passivateCompleted / sendMsgBuffer :388-400,
:437-466).

  an entity type is a range of unregistered ids with a kind, start state, stop message and idle timeout; tick t --
    1. formation: the inbox of §2.7.  For an entity that is not alive: the messages its last plain stop left queued
       (they head its inbox) and every item whose sender is the entity itself are dead letters; if anything stays it
       starts -- kind, word 0 = base, word 1 as declared, the idle timeout set at t, started++, incarnations++, and
       restarted++ when it stopped while passivating in tick t - 1 -- and the rest is its inbox;
    2. admission and drain unchanged;
    3. A_PASSIVATE by an entity that is not passivating: marked, the type's stop payload to the entity itself (an
       ordinary emission), passivations++; by a passivating one: passivate_ignored++; by any other actor:
       passivate_unknown++;
    4. a stop while passivating: passivated++, and the rest of the admitted inbox stays queued (no dead letter); any
       other stop is §2.7's, and the number of messages it leaves queued is remembered for the next formation;
    5. any stop clears the mark.

With no entity type it is ReceiveTimeoutModel.
"""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, STOPPED, UNHANDLED
from tests.receive_timeout_model import TAG_RT, ReceiveTimeoutModel
from tests.timer_model import GEN_MASK, MAX_DELAY, NONE, TAG_TIMER, clamp_delay

SHARD_KEYS = ("started", "restarted", "passivations", "passivated", "passivate_ignored", "passivate_unknown")


class ShardingModel(ReceiveTimeoutModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.types = []          # (first, count, kind, base, word1 or None, stop payload, idle delay, idle payload)
        self.sh = dict.fromkeys(SHARD_KEYS, 0)
        self.inc = self.passivating = self.pst = self.held = None
        self._passivate = False  # the case that runs holds A_PASSIVATE

    # ------------------------------------------------------------ setup
    def set_sharding(self, types):
        assert self.rt_on and not self.types, "on top of the receive timeouts, once"
        types = [tuple(t) for t in types]
        assert 1 <= len(types) <= 8
        for i, (f, c, *_r) in enumerate(types):
            assert c > 0 and f + c <= self.n and not self.alive[f:f + c].any(), "an entity range holds unregistered ids"
            assert all(f + c <= g or g + d <= f for g, d, *_s in types[:i]), "entity ranges are disjoint"
        self.types = types
        self.inc, self.passivating = [0] * self.n, [0] * self.n
        self.pst, self.held = [0] * self.n, [0] * self.n

    def register_range(self, first, count, kind, init_state=None):
        assert all(first + count <= f or f + c <= first for f, c, *_r in self.types) or not count, "an entity range"
        super().register_range(first, count, kind, init_state)

    def _type_of(self, a):
        for t in self.types:
            if t[0] <= a < t[0] + t[1]:
                return t
        return None

    # ------------------------------------------------------------ reading
    def sharding_info(self) -> dict:
        alive = sum(int(self.alive[f:f + c].sum()) for f, c, *_r in self.types)
        return dict(self.sh, alive=alive)

    def read_entities(self, first=0, count=None) -> dict:
        count = self.n - first if count is None else count
        o = dict(alive=np.zeros(count, np.uint32), incarnations=np.zeros(count, np.uint32), passivating=np.zeros(count, np.uint32))
        for i in range(count):
            o["alive"][i] = self.alive[first + i] & 1
            if self.types:
                o["incarnations"][i] = self.inc[first + i]
                o["passivating"][i] = self.passivating[first + i]
        return o

    # ------------------------------------------------------------ behaviours
    def _compiled(self, a, w, src, pay):
        if not self.types:
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
                elif A.op == typed.A_PASSIVATE:
                    self._passivate = True
            if C.result == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME
            return C.result
        return UNHANDLED

    def _passivated(self, a):
        """shard ! Passivate(a) (Shard.passivate :405-417)"""
        ty = self._type_of(a)
        if ty is None:
            self.sh["passivate_unknown"] += 1
        elif self.passivating[a]:
            self.sh["passivate_ignored"] += 1
        else:
            self.passivating[a] = 1
            self._emit(a, a, ty[5])
            self.sh["passivations"] += 1

    # ------------------------------------------------------------ supersteps
    def step(self) -> bool:
        if not self.types:
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
            sizes[a] = len(q)
            ty = self._type_of(a)
            if not self.alive[a] and ty is not None:  # getOrCreateEntity (:504-516)
                old, self.held[a] = self.held[a], 0
                stay = [(s, p) for i, (s, p) in enumerate(q) if i >= old and s != a]
                self.c["dead_letters"] += len(q) - len(stay)
                q = stay
                if q:
                    self.alive[a] = 1
                    self.kind[a] = ty[2]
                    self.words[a, 0] = ty[3]
                    self.words[a, 1] = a if ty[4] is None else ty[4]
                    if ty[6]:
                        self.rt_delay[a], self.rt_pay[a] = min(int(ty[6]), MAX_DELAY), ty[7] & M32
                        self.rt_next[a] = self.now + self.rt_delay[a]
                    self.inc[a] += 1
                    self.sh["started"] += 1
                    self.sh["restarted"] += self.pst[a] != 0 and self.pst[a] == self.now - 1
            L = len(q)
            if not self.alive[a]:
                self.c["dead_letters"] += L
                continue
            C, T = self._limits(a)
            keep = L if C == 0 else min(L, C)
            self.c["dead_letters"] += L - keep
            adm = q[:keep]
            nd = min(keep, T)
            w = [int(self.words[a, 0]), int(self.words[a, 1])]
            taken = nd  # the messages of the admitted inbox that do not stay queued
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
                self._passivate = False
                r = self._apply(a, w, sv, pv)
                if self._passivate:
                    self._passivated(a)
                delay, pay, changed = self._cur
                if changed:
                    self.rt_delay[a] = delay
                    if delay:
                        self.rt_pay[a] = pay
                if r == UNHANDLED:
                    self.c["unhandled"] += 1
                if r == STOPPED:
                    self.alive[a] = 0
                    if ty is not None and self.passivating[a]:  # passivateCompleted (:453-466): the buffer stays
                        self.passivating[a] = 0
                        self.pst[a] = self.now
                        self.sh["passivated"] += 1
                        taken = i + 1
                    else:
                        self.c["dead_letters"] += nd - i - 1
                        if ty is not None:
                            self.held[a] = keep - nd
                    for k in range(self.n_keys):
                        self._cancel(a, k)
                    self.rt_delay[a], self.rt_next[a] = 0, NONE
                    break
                if changed or (self.rt_delay[a] and (envelope or (pv >> 24) not in self.transparent)):
                    self.rt_next[a] = self.now + self.rt_delay[a] if self.rt_delay[a] else NONE
            self.words[a, 0], self.words[a, 1] = w[0], w[1]
            self.backlog += [(a, s, p) for s, p in adm[taken:]]
        self.emitted_q, self.staged_q = self._out, []
        self.inbox_sizes.append(sizes)
        if msgs:
            self.c["supersteps"] += 1
        return True
