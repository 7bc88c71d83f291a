"""A pure Python model of one dispatcher of the engine with death watch: DESIGN.md §2 (the BSP superstep,
tests/prio_model.PrioModel) plus §2.4 (context.watch / watchWith / unwatch and the Terminated signal; the
reference: AA/dungeon/DeathWatch.scala:19-113,147-162, TY/internal/adapter/ActorAdapter.scala:84-91,134-138,
200-205, pinned by WatchSpec.scala:54-85,196-362).

  one superstep is one tick; tick t --
    0. the engine is active at the entry of t iff mail is in flight, or a slot is due, or an actor stopped in
       t - 1 while a slot of the engine was watching at the end of t - 1; else the run ends;
    1. every due slot becomes notified; inbox = backlog ++ arrivals emitted in t - 1 (canonical order) ++
       host-staged tells ++ the tick's Terminated envelopes in (actor, slot) order;
    2. admission by position, drain of the first min(len, T) -- unchanged;
    3. a drained message with tag 0xFE is a Terminated envelope: it counts as delivered; slot not notified or
       another generation (mod 2^22) -> discarded; else the slot becomes free and the custom message runs the
       ordinary cases, a plain Terminated the signal cases (sender = the watchee); no signal case matches ->
       the death pact: the actor stops;
    4. a stop frees the actor's slots and sets its death tick to t;
    5. at the end of t every watching slot whose watchee's death tick is <= t - 1 becomes due.

It takes the same calls as GpuEngine, so with no watch in use it is pinned to the frozen oracle.
"""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, STOPPED, UNHANDLED, PrioModel

NONE = 0xFFFFFFFF
TAG_WATCH = 0xFE
GEN_MASK = (1 << 22) - 1
FREE, WATCHING, DUE, NOTIFIED, HAS_MSG = 0, 1, 2, 3, 4
INFO_KEYS = ("watches", "terminated", "discarded", "death_pacts", "conflicts", "watching", "pending", "ticks")


class Slot:
    __slots__ = ("state", "wee", "has", "payload", "gen")

    def __init__(self):
        self.state, self.wee, self.has, self.payload, self.gen = FREE, 0, False, 0, 0


class SlotsExhausted(Exception):
    """a watch found no free slot (the engine: sticky AGX_ECAPACITY)"""


class WatchModel(PrioModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n_slots = 0
        self.slots = None        # [actor][slot]
        self.died = None         # the actor's death tick, NONE while alive
        self.now = 0             # ticks run so far
        self.started = False
        self.stop_tick = NONE    # the last tick in which an actor stopped
        self.any_tick = NONE     # the last tick at whose end a slot was watching
        self.full = False        # a watch found no free slot
        self.w = dict(watches=0, terminated=0, discarded=0, death_pacts=0, conflicts=0, ticks=0)

    # ------------------------------------------------------------ setup
    def set_death_watch(self, n_slots: int):
        assert 1 <= n_slots <= 4 and self.kmax == 1
        self.n_slots = n_slots
        self.slots = [[Slot() for _ in range(n_slots)] for _ in range(self.n)]
        self.died = [NONE] * self.n

    def _sync_died(self):
        """an actor that is not alive and has no death tick: never registered (before the first run: dead before
        tick 1) or stopped from outside (dead in the current tick)"""
        for a in range(self.n):
            if not self.alive[a] and self.died[a] == NONE:
                self.died[a] = self.now if self.started else 0

    def _watch(self, a, x, with_, m):
        """-> (conflict, the slot occupied now or None)"""
        x &= M32
        if x == a:
            return False, None
        free = None
        for k, s in enumerate(self.slots[a]):
            if s.state == FREE:
                if free is None:
                    free = k
            elif s.wee == x:
                if s.state == NOTIFIED:
                    return False, None
                return not (s.has == with_ and (not with_ or s.payload == (m & M32))), None
        if free is None:
            self.full = True
            return False, None
        s = self.slots[a][free]
        s.state, s.wee, s.has, s.payload = WATCHING, x, with_, (m & M32) if with_ else 0
        s.gen += 1
        self.w["watches"] += 1
        return False, free

    def _unwatch(self, a, x):
        x &= M32
        for s in self.slots[a]:
            if s.state != FREE and s.wee == x:
                s.state, s.has = FREE, False

    def _stop(self, a):
        for s in self.slots[a]:
            s.state, s.has = FREE, False
        self.died[a] = self.now
        self.stop_tick = self.now

    def _dead(self, x) -> bool:
        return x >= self.n or self.died[x] != NONE

    def _any_watching(self) -> bool:
        return any(s.state == WATCHING for row in self.slots for s in row)

    def start_watch(self, first, count, watchees=None, *, offset=0, message=None):
        assert self.n_slots
        self._sync_died()
        new = []
        for i in range(count):
            a = first + i
            if not self.alive[a]:
                continue
            x = int(watchees[i]) if watchees is not None else (a + offset) % self.n
            conflict, k = self._watch(a, x, message is not None, message or 0)
            if conflict:
                self.alive[a] = 0
                self._stop(a)
                self.w["conflicts"] += 1
            elif k is not None:
                new.append((a, k))
        for a, k in new:  # a watchee that is dead by now: due at once
            s = self.slots[a][k]
            if s.state == WATCHING and self._dead(s.wee):
                s.state = DUE
        if self._any_watching():
            self.any_tick = self.now
        if self.full:
            raise SlotsExhausted()

    def tell(self, dst, payload, src=None):
        if self.n_slots:
            assert not np.any((np.atleast_1d(np.asarray(payload, np.uint32)) >> 24) == TAG_WATCH), "tag 0xFE is reserved"
        super().tell(dst, payload, src)

    # ------------------------------------------------------------ reading
    def watch_info(self) -> dict:
        nw = npd = 0
        if self.slots:
            for row in self.slots:
                for s in row:
                    nw += s.state == WATCHING
                    npd += s.state == DUE
        return dict(self.w, watching=int(nw), pending=int(npd))

    def read_watch(self, a) -> dict:
        o = {k: np.zeros(4, np.uint32) for k in ("watchee", "state", "payload", "generation")}
        for k in range(self.n_slots):
            s = self.slots[a][k]
            o["watchee"][k] = s.wee
            o["state"][k] = s.state | (HAS_MSG if s.has else 0)
            o["payload"][k] = s.payload
            o["generation"][k] = s.gen & M32
        return o

    # ------------------------------------------------------------ behaviours
    def _compiled_w(self, a, w, src, pay, signal):
        """-> (result, conflict)"""
        t = self.tables
        b = int(self.kind[a]) - typed.KIND_COMPILED
        if t is None or b >= t.n_behaviors:
            return UNHANDLED, False
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
                d = 0
                if A.op == typed.A_TELL or A.op >= typed.A_WATCH:
                    if A.dsrc == typed.V_SELF:
                        d = (a + A.dk) % self.n
                    else:
                        d = self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a)
                    d = min(d, M32)
                msg = ((v & 0xFFFFFF) | A.or_mask) if A.or_mask else (v & M32)
                if A.op == typed.A_SET:
                    w[x] = v
                elif A.op == typed.A_ADD:
                    w[x] = (w[x] + v) & M64
                elif A.op == typed.A_MAX:
                    w[x] = max(w[x], v)
                elif A.op == typed.A_MIN:
                    w[x] = min(w[x], v)
                elif A.op == typed.A_TELL:
                    self._emit(a, d, msg)
                elif A.op in (typed.A_WATCH, typed.A_WATCH_WITH):
                    conflict, _ = self._watch(a, d, A.op == typed.A_WATCH_WITH, msg)
                    if conflict:  # IllegalStateException: the rest of the case is skipped, the actor stops
                        return STOPPED, True
                elif A.op == typed.A_UNWATCH:
                    self._unwatch(a, d)
            res = C.result & ~typed.CASE_SIGNAL
            if res == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME, False
            return res, False
        return UNHANDLED, False

    # ------------------------------------------------------------ supersteps
    def _active(self) -> bool:
        if self.backlog or self.emitted_q or self.staged_q:
            return True
        if any(s.state == DUE for row in self.slots for s in row):
            return True
        return self.stop_tick == self.now and self.any_tick == self.now

    def step(self) -> bool:
        if not self.n_slots:
            return super().step()
        self._sync_died()
        if not self._active():
            return False
        self.started = True
        self.now += 1
        self.w["ticks"] += 1
        envs = []
        for a in range(self.n):
            for k, s in enumerate(self.slots[a]):
                if s.state == DUE:
                    s.state = NOTIFIED
                    envs.append((a, s.wee, (TAG_WATCH << 24) | (k << 22) | (s.gen & GEN_MASK)))
        self.w["terminated"] += len(envs)
        msgs = self.backlog + self.emitted_q + self.staged_q + envs
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
                sig = False
                if pv >> 24 == TAG_WATCH:  # receivedTerminated
                    k = (pv >> 22) & 3
                    s = self.slots[a][k] if k < self.n_slots else None
                    if s is None or s.state != NOTIFIED or (s.gen ^ pv) & GEN_MASK:
                        self.w["discarded"] += 1
                        continue
                    sig = not s.has
                    sv, pv = s.wee, (typed.SIGNAL_TERMINATED if sig else s.payload)
                    s.state, s.has = FREE, False
                conflict = False
                if int(self.kind[a]) >= typed.KIND_COMPILED:
                    r, conflict = self._compiled_w(a, w, sv, pv, sig)
                else:
                    r = UNHANDLED if sig else self._apply(a, w, sv, pv)
                if sig and r == UNHANDLED:  # the death pact
                    r = STOPPED
                    self.w["death_pacts"] += 1
                if conflict:
                    self.w["conflicts"] += 1
                if r == UNHANDLED:
                    self.c["unhandled"] += 1
                if r == STOPPED:
                    self.alive[a] = 0
                    self.c["dead_letters"] += nd - i - 1
                    self._stop(a)
                    break
            self.words[a, 0], self.words[a, 1] = w[0], w[1]
            self.backlog += [(a, s, p) for s, p in adm[nd:]]
        self.emitted_q, self.staged_q = self._out, []
        self.inbox_sizes.append(sizes)
        if msgs:
            self.c["supersteps"] += 1
        for row in self.slots:  # the end of the tick: a death of an earlier tick answers its watching slots
            for s in row:
                if s.state == WATCHING and (s.wee >= self.n or self.died[s.wee] < self.now):
                    s.state = DUE
        if self._any_watching():
            self.any_tick = self.now
        if self.full:
            raise SlotsExhausted()
        return True
