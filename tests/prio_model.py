"""A pure Python model of one dispatcher of the engine, with priority mailboxes: a direct restatement
of DESIGN.md §2 (the BSP superstep) plus §2.1 (the order step of a prioritised mailbox class).

It takes the same calls as GpuEngine / BspOracle (Workload.apply_to installs a workload into it), so
the tests pin it to the frozen FIFO oracle with no tables set, and use it as the reference for the
new semantics with tables (Mailbox.scala:726-816 priority / stable priority, :867-1025
control-aware):

  superstep s, per actor with mail --
    1. inbox = backlog in its stored order, then arrivals in canonical order (sender id, emission
       index), then staged tells;
    2. admission by arrival position: position p is admitted iff C == 0 or p < C (the backlog counts);
    3. order: a class with a table stably sorts the admitted messages by prio[payload >> 24];
    4. drain the first min(len, max(T, 1)) of that order, T clamped to C; a stop ends the drain and
       the rest of it are dead letters;
    5. the backlog is the rest, stored in that order.

Single rank, plain and compiled behaviours only (no CRDT kinds).  Not fast; not meant to be.
"""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from akka_amd.engine import Kind

M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
SAME, STOPPED, UNHANDLED, BECOME = 0, 1, 2, 3
MAX_CLASSES = 8


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def fanout_rand(seed: int, self_id: int, h: int, j: int) -> int:
    return splitmix64(seed ^ splitmix64(((self_id << 32) ^ (h << 4) ^ j) & M64))


class PrioModel:
    def __init__(self, n_actors: int, throughput: int = 5, capacity: int = 0, n_words: int = 2, max_emit: int = 1,
                 **_layout):
        assert n_words == 2, "the model keeps state words 0 and 1"
        self.n = int(n_actors)
        self.Tr = max(int(throughput), 1)
        self.kmax = max_emit
        self.kind = np.zeros(self.n, np.int64)
        self.alive = np.zeros(self.n, np.uint8)
        self.words = np.zeros((self.n, 2), np.uint64)
        self.mcap = [int(capacity)] + [None] * (MAX_CLASSES - 1)
        self.mcls = np.zeros(self.n, np.int64)
        self.prio = {}            # class -> 256 priorities
        self.host_lo, self.host_n = 0, 0
        self.ring_stride = 1
        self.fan = None           # (k, seed, cdf, perm)
        self.graph = None         # (row_ptr, col)
        self.tables = None
        self.backlog, self.emitted_q, self.staged_q = [], [], []
        self.outbox = []          # (dst, src, payload) in canonical emission order
        self.c = dict(delivered=0, dead_letters=0, unhandled=0, emitted=0, staged=0, supersteps=0, in_flight=0)
        self.inbox_sizes = []     # per superstep: messages per destination actor (bucket load checks)

    # ------------------------------------------------------------ the engine's setup calls
    def register_range(self, first, count, kind, init_state=None):
        self.kind[first:first + count] = kind
        self.alive[first:first + count] = 1 if kind != Kind.NONE else 0
        st = np.zeros((count, 2), np.uint64)
        if init_state is not None:
            a = np.asarray(init_state, dtype=np.uint64).reshape(count, -1)[:, :2]
            st[:, :a.shape[1]] = a
        self.words[first:first + count] = st

    def set_mailbox_class(self, cls, capacity):
        assert 0 < cls < MAX_CLASSES
        self.mcap[cls] = int(capacity)

    def set_mailbox(self, first, count, cls):
        assert self.mcap[cls] is not None, "class not configured"
        self.mcls[first:first + count] = cls

    def set_mailbox_priority(self, cls, table):
        assert self.mcap[cls] is not None, "class not configured"
        if table is None:
            self.prio.pop(cls, None)
            return
        t = [int(x) for x in (bytes(table) if isinstance(table, (bytes, bytearray)) else table)]
        assert len(t) == 256 and all(0 <= x <= 255 for x in t)
        self.prio[cls] = t

    def set_outbound(self, first_host_id, n_host, capacity=1 << 20):
        self.host_lo, self.host_n = int(first_host_id), int(n_host)

    def set_ring(self, stride=1):
        self.ring_stride = int(stride)

    def set_fanout(self, k, seed, cdf, perm):
        self.fan = (int(k), int(seed), np.asarray(cdf, np.uint32), np.asarray(perm, np.uint32))

    def set_graph(self, row_ptr, col):
        self.graph = (np.asarray(row_ptr, np.uint64), np.asarray(col, np.uint32))

    def set_behaviors(self, tables):
        self.tables = tables

    def tell(self, dst, payload, src=None):
        dst = np.atleast_1d(np.asarray(dst, dtype=np.uint32))
        pay = np.broadcast_to(np.asarray(payload, dtype=np.uint32), dst.shape)
        s = np.full(dst.shape, M32, np.uint32) if src is None else np.broadcast_to(np.asarray(src, np.uint32), dst.shape)
        for d, sv, p in zip(dst.tolist(), s.tolist(), pay.tolist()):
            self.c["staged"] += 1
            if d >= self.n:
                self.c["dead_letters"] += 1  # (a host tell to an unknown ref)
                continue
            self.staged_q.append((d, sv, p))

    def take_outbound(self):
        o = np.asarray(self.outbox, dtype=np.uint32).reshape(-1, 3)
        self.outbox = []
        return o[:, 0].copy(), o[:, 1].copy(), o[:, 2].copy()

    def read_state(self):
        return self.words.copy(), self.alive.copy()

    def close(self):
        pass

    # ------------------------------------------------------------ behaviours
    def _emit(self, self_id, dst, pay):
        dst &= M32
        pay &= M32
        if dst >= self.n and 0 <= dst - self.host_lo < self.host_n:  # a host-side actor: the outbox
            self.outbox.append((dst, self_id, pay))
            return
        self.c["emitted"] += 1
        if dst >= self.n:
            self.c["dead_letters"] += 1
            return
        self._out.append((dst, self_id, pay))

    def _operand(self, src, word, k, pay, w, sender, self_id):
        b = (0, pay, pay >> 24, pay & 0xFFFFFF, w[word & 1], sender, self_id)[src] if src <= typed.V_SELF else 0
        return (b + k) & M64

    @staticmethod
    def _cmp(op, a, b):
        return (True, a == b, a != b, a < b, a <= b, a > b, a >= b)[op] if op <= typed.CMP_GE else True

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
            for i in range(C.act_first, C.act_first + C.act_count):
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
            if C.result == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME
            return C.result
        return UNHANDLED

    def _apply(self, a, w, src, pay):
        kind = int(self.kind[a])
        if kind >= typed.KIND_COMPILED:
            return self._compiled(a, w, src, pay)
        if kind == Kind.COUNTER:
            w[0] = (w[0] + 1) & M64
            w[1] = (w[1] + pay) & M64
        elif kind == Kind.RING:
            w[0] = (w[0] + 1) & M64
            if pay > 0:
                self._emit(a, (a + self.ring_stride % self.n) % self.n, pay - 1)
        elif kind == Kind.FANOUT:
            w[0] = (w[0] + 1) & M64
            w[1] = (w[1] + pay) & M64
            ttl, h = pay >> 24, pay & 0xFFFFFF
            if ttl > 0:
                k, seed, cdf, perm = self.fan
                for j in range(k):
                    r = fanout_rand(seed, a, h, j)
                    i = min(int(np.searchsorted(cdf, r >> 32, side="left")), cdf.size - 1)
                    self._emit(a, int(perm[i]), ((ttl - 1) << 24) | (r & 0xFFFFFF))
        elif kind == Kind.FORWARD_RR:
            w[0] = (w[0] + 1) & M64
            if pay > 0:
                row, col = self.graph
                b0, deg = int(row[a]), int(row[a + 1]) - int(row[a])
                if deg:
                    e = b0 + w[1] % deg
                    w[1] = (w[1] + 1) & M64
                    self._emit(a, int(col[e]), pay - 1)
        elif kind == Kind.STOP_AFTER:
            w[0] = (w[0] + 1) & M64
            return STOPPED if w[0] >= w[1] else SAME
        elif kind == Kind.PINGPONG:
            res = STOPPED if w[0] == 0 else SAME
            w[1] = (w[1] + 1) & M64
            self._emit(a, src, pay)
            w[0] = (w[0] - 1) & M64
            return res
        elif kind == Kind.EVEN:
            if pay & 1:
                return UNHANDLED
            w[0] = (w[0] + 1) & M64
        return SAME

    # ------------------------------------------------------------ supersteps
    def _limits(self, a):
        C = self.mcap[int(self.mcls[a])]
        return C, (min(self.Tr, C) if C else self.Tr)

    def step(self) -> bool:
        msgs = self.backlog + self.emitted_q + self.staged_q
        if not msgs:
            return False
        inbox = {}
        for d, s, p in msgs:  # (stable: each actor's messages keep the list's order)
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
            keep = L if C == 0 else min(L, C)          # admission by arrival position
            self.c["dead_letters"] += L - keep
            adm = q[:keep]
            tab = self.prio.get(int(self.mcls[a]))
            if tab is not None:                           # the order step (stable)
                adm = sorted(adm, key=lambda m: tab[m[1] >> 24])
            nd = min(keep, T)
            w = [int(self.words[a, 0]), int(self.words[a, 1])]
            for i in range(nd):
                r = self._apply(a, w, adm[i][0], adm[i][1])
                self.c["delivered"] += 1
                if r == UNHANDLED:
                    self.c["unhandled"] += 1
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

    def run(self, max_supersteps: int = 1 << 30) -> dict:
        i = 0
        while i < max_supersteps and self.step():
            i += 1
        self.c["in_flight"] = len(self.backlog) + len(self.emitted_q) + len(self.staged_q)
        return dict(self.c)

    def max_bucket_inbox(self, bucket_actors: int) -> int:
        """The largest inbox (backlog included) any bucket of `bucket_actors` actors saw so far."""
        best = 0
        for s in self.inbox_sizes:
            pad = (-s.size) % bucket_actors
            best = max(best, int(np.pad(s, (0, pad)).reshape(-1, bucket_actors).sum(axis=1).max()))
        return best


def per_sender(d, s, p):
    """outbox -> canonical per-sender sequences (a stable sort by sender keeps each sender's order)"""
    o = np.argsort(s, kind="stable")
    return np.stack([s[o], d[o], p[o]])
