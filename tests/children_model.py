"""A pure Python model of one dispatcher of the engine with children: tests/watch_model.WatchModel (DESIGN.md
§2.4) plus §2.6 -- context.spawn, context.stop(child) and the parent's stop taking its children (the reference:
AA/dungeon/Children.scala, TY/internal/adapter/ActorContextAdapter.scala:79-106, pinned by
ActorContextSpec.scala:214-240,336-428,656-, GracefulStopSpec.scala:20-48, RoutersSpec.scala:40-104).

  tick t, beside WatchModel's steps --
    1a. the tick's Create and Stop envelopes (tags 0xFD, 0xFC) leave the inbox before admission and count as
        delivered: per actor all Creates in inbox order, then all Stops.  A Create from the id's computed parent,
        for an id never created, with a valid site: the actor is born (alive, the site's kind and state).  A Stop
        from the computed parent to a live created child: it stops (death tick t, slots freed; its mail of the
        tick is dead letters).  Every other one is discarded;
    5a. at the end of t, if an actor stopped in t - 1, every live created child whose computed parent has a
        death tick <= t - 1 stops (death tick t); then WatchModel's step 5;
    0.  the engine is active also if an actor stopped in t - 1 while a created child was alive at the end of t - 1.

With no region set, or regions and no spawn, it is WatchModel bit for bit.
"""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, STOPPED, UNHANDLED
from tests.watch_model import DUE, NONE, NOTIFIED, FREE, TAG_WATCH, GEN_MASK, WATCHING, SlotsExhausted, WatchModel

TAG_CREATE, TAG_STOP = 0xFD, 0xFC
ARG_BITS, ARG_MASK, MAX_SITES, MAX_REGIONS = 18, (1 << 18) - 1, 64, 8
CHILD_KEYS = ("spawned", "refused", "created", "child_stops", "cascade_stops", "illegal_stops", "discarded", "live")


class ChildrenModel(WatchModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.regions = []   # (first_parent, n_parents, first_child, max_children)
        self.sites = []     # (kind, word-0 base, word-1 constant or None for the parent's id)
        self.spawn_count = np.zeros(self.n, np.int64)
        self.created = np.zeros(self.n, bool)
        self.stops_in = set()  # the ticks in which an actor stopped
        self.ch = dict(spawned=0, refused=0, created=0, child_stops=0, cascade_stops=0, illegal_stops=0, discarded=0)

    # ------------------------------------------------------------ setup
    def set_children(self, regions, sites):
        assert self.n_slots and not self.started
        self.regions = [tuple(int(x) for x in r) for r in regions]
        self.sites = [(int(k), int(b), None if w1 is None else int(w1)) for k, b, w1 in sites]
        for fp, npar, fc, mc in self.regions:  # death tick "none", not "dead before tick 1"
            for x in range(fc, fc + npar * mc):
                assert not self.alive[x]
                self.died[x] = NONE

    def _sync_died(self):
        for a in range(self.n):
            if not self.alive[a] and self.died[a] == NONE and self.parent_of(a) == NONE:
                self.died[a] = self.now if self.started else 0

    def parent_of(self, x) -> int:
        for fp, npar, fc, mc in self.regions:
            if fc <= x < fc + npar * mc:
                return fp + (x - fc) // mc
        return NONE

    def _block_of(self, p):
        for fp, npar, fc, mc in self.regions:
            if fp <= p < fp + npar:
                return fc + (p - fp) * mc, mc
        return None

    def _spawn(self, p) -> int:
        blk = self._block_of(p)
        k = int(self.spawn_count[p])
        if blk is None or k >= blk[1]:
            self.ch["refused"] += 1
            return NONE
        self.spawn_count[p] = k + 1
        self.ch["spawned"] += 1
        return blk[0] + k

    def _own_child(self, p, x) -> bool:
        blk = self._block_of(p)
        return blk is not None and blk[0] <= x < blk[0] + int(self.spawn_count[p])

    def _child_at(self, p, i) -> int:
        blk, k = self._block_of(p), int(self.spawn_count[p])
        return NONE if blk is None or not k else blk[0] + i % k

    def spawn_children(self, first, count, site, arg=0):
        assert self.regions
        self._sync_died()
        for p in range(first, first + count):
            if not self.alive[p]:
                continue
            ch = self._spawn(p)
            if ch != NONE:
                self.c["staged"] += 1
                self.staged_q.append((ch, p, (TAG_CREATE << 24) | (site << ARG_BITS) | (arg & ARG_MASK)))

    def tell(self, dst, payload, src=None):
        if self.regions:
            tag = np.atleast_1d(np.asarray(payload, np.uint32)) >> 24
            assert not np.any((tag == TAG_CREATE) | (tag == TAG_STOP)), "tags 0xFD / 0xFC are reserved"
        super().tell(dst, payload, src)

    # ------------------------------------------------------------ reading
    def children_info(self) -> dict:
        return dict(self.ch, live=int(sum(1 for a in range(self.n) if self.created[a] and self.alive[a])))

    def read_children(self, a) -> dict:
        return dict(parent=self.parent_of(a), spawn_count=int(self.spawn_count[a]), created=int(self.created[a]))

    # ------------------------------------------------------------ behaviours
    def _operand(self, src, word, k, pay, w, sender, self_id):
        if src == typed.V_SPAWNED:
            return (int(self.spawn_count[self_id]) + k) & M64
        if src == typed.V_CHILD:
            return self._child_at(self_id, ((w[word] if word <= 1 else 0) + k) & M64)
        return super()._operand(src, word, k, pay, w, sender, self_id)

    def _compiled_c(self, a, w, src, pay, signal):
        """-> (result, conflict, illegal)"""
        t = self.tables
        b = int(self.kind[a]) - typed.KIND_COMPILED
        if t is None or b >= t.n_behaviors:
            return UNHANDLED, False, False
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
                if A.op == typed.A_TELL or (A.op >= typed.A_WATCH and A.op != typed.A_SPAWN):
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
                    if conflict:
                        return STOPPED, True, False
                elif A.op == typed.A_UNWATCH:
                    self._unwatch(a, d)
                elif A.op == typed.A_SPAWN:
                    ch = self._spawn(a)
                    if A.pad0 & 1:
                        w[x] = ch
                    if ch != NONE:
                        self._emit(a, ch, (TAG_CREATE << 24) | ((A.dword & (MAX_SITES - 1)) << ARG_BITS) | (v & ARG_MASK))
                elif A.op == typed.A_STOP_CHILD:
                    if not self._own_child(a, d):  # IllegalArgumentException: the rest is skipped, the actor stops
                        return STOPPED, False, True
                    self._emit(a, d, TAG_STOP << 24)
            res = C.result & ~typed.CASE_SIGNAL
            if res == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME, False, False
            return res, False, False
        return UNHANDLED, False, False

    def _stop(self, a):
        super()._stop(a)
        self.stops_in.add(self.now)

    # ------------------------------------------------------------ supersteps
    def _live_children(self) -> bool:
        return bool(np.any(self.created & (self.alive != 0)))

    def _control(self, a, q):
        """the tick's Create and Stop envelopes of actor a leave its inbox `q`; -> the rest"""
        rest = [m for m in q if m[1] >> 24 not in (TAG_CREATE, TAG_STOP)]
        if len(rest) == len(q):
            return q
        par = self.parent_of(a)
        self.c["delivered"] += len(q) - len(rest)
        for s, p in q:
            if p >> 24 != TAG_CREATE:
                continue
            site = (p >> ARG_BITS) & (MAX_SITES - 1)
            if par != NONE and s == par and not self.created[a] and site < len(self.sites):
                kind, base, w1 = self.sites[site]
                self.created[a] = True
                self.alive[a] = 1
                self.kind[a] = kind
                self.words[a, 0] = (base + (p & ARG_MASK)) & M64
                self.words[a, 1] = par if w1 is None else w1
                self.ch["created"] += 1
            else:
                self.ch["discarded"] += 1
        stopped = False
        for s, p in q:
            if p >> 24 != TAG_STOP:
                continue
            if par != NONE and s == par and self.created[a] and self.alive[a] and not stopped:
                stopped = True
                self.alive[a] = 0
                self._stop(a)
                self.ch["child_stops"] += 1
            else:
                self.ch["discarded"] += 1
        return rest

    def step(self) -> bool:
        if not self.regions:
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
            sizes[a] = len(q)
            q = self._control(a, q)
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
                conflict = illegal = False
                if int(self.kind[a]) >= typed.KIND_COMPILED:
                    r, conflict, illegal = self._compiled_c(a, w, sv, pv, sig)
                else:
                    r = UNHANDLED if sig else self._apply(a, w, sv, pv)
                if sig and r == UNHANDLED:  # the death pact
                    r = STOPPED
                    self.w["death_pacts"] += 1
                if conflict:
                    self.w["conflicts"] += 1
                if illegal:
                    self.ch["illegal_stops"] += 1
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
        if self.now - 1 in self.stops_in:  # a parent's stop takes its children, one level per tick
            for a in range(self.n):
                if self.created[a] and self.alive[a]:
                    p = self.parent_of(a)
                    if p != NONE and self.died[p] != NONE and self.died[p] < self.now:
                        self.alive[a] = 0
                        self._stop(a)
                        self.ch["cascade_stops"] += 1
        for row in self.slots:  # the end of the tick: a death of an earlier tick answers its watching slots
            for s in row:
                if s.state == WATCHING and (s.wee >= self.n or self.died[s.wee] < self.now):
                    s.state = DUE
        if self._any_watching() or self._live_children():
            self.any_tick = self.now
        if self.full:
            raise SlotsExhausted()
        return True
