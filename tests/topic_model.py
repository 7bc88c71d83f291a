"""A pure Python model of an engine with pub-sub topics: ReceptionistModel plus DESIGN.md §2.10,
in plain Python.

  * a topic is a service key: subscribing is registering, a stop unsubscribes;
  * a publish action run by actor p while it drains message q of its window in tick s is logged as
    (key, payload, sender = p); the tick's log is ordered by (p, q); host publications are appended in call order;
  * when the inbox of tick s + 1 is formed, every entry of the log goes to every actor whose bit `key` is set at that
    moment, ascending ids per entry, after the backlog, the arrivals and the host-staged tells; admission is by
    position as for any mail;
  * a publication that finds no recipient is counted (`no_subscribers`), neither emitted nor a dead letter;
  * planned deliveries are in flight: staged + emitted + fanned_out = delivered + dead_letters + in_flight;
  * a tick is a superstep with mail: a log without recipients waits for the next tick.

Not fast; not meant to be."""
from __future__ import annotations

from bisect import bisect_left

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, UNHANDLED
from tests.receptionist_model import NONE, ReceptionistModel

TOPIC_INFO_KEYS = ("published", "fanned_out", "no_subscribers", "host_published")
NO_SENDER = 0xFFFFFFFF


class TopicModel(ReceptionistModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.log_cap = 0
        self.tlog = []      # the pending log: (key, sender, payload) in delivery order
        self._pubs = []     # the publications of the tick being drained: (publisher, window index, key, payload)
        self._at = (None, 0)  # the actor being drained and the index of its message within the window
        self.tinfo = dict.fromkeys(TOPIC_INFO_KEYS, 0)  # (fanned_out / no_subscribers: of the logs consumed so far)
        self.topic_error = False
        self.delivery_dead_letters = 0

    # ------------------------------------------------------------ the engine's calls
    def set_topics(self, log_capacity=1024):
        assert self.n_keys, "topics need the receptionist"
        assert 1 <= log_capacity <= 65536 and not self.log_cap
        self.log_cap = int(log_capacity)

    def publish(self, key, payload, sender=NO_SENDER):
        assert self.log_cap and key < self.n_keys
        self.tinfo["host_published"] += 1
        if len(self.tlog) >= self.log_cap:
            self.topic_error = True
            return
        self.tlog.append((int(key), int(sender) & M32, int(payload) & M32))

    def _plan(self):
        """the deliveries of the pending log against the masks as they are now, and its entries without a recipient"""
        out, nosub = [], 0
        for k, s, p in self.tlog:
            ids = np.flatnonzero((self.mask >> k) & 1).tolist()
            nosub += not ids
            out += [(a, s, p) for a in ids]
        return out, nosub

    def topic_info(self):
        d = dict(self.tinfo)
        planned, nosub = self._plan()
        d["fanned_out"] += len(planned)
        d["no_subscribers"] += nosub
        return d

    def read_topic_log(self):
        return np.asarray(self.tlog, np.uint32).reshape(-1, 3)

    # ------------------------------------------------------------ behaviours
    def _apply(self, a, w, src, pay):
        self._at = (a, self._at[1] + 1 if self._at[0] == a else 0)
        return super()._apply(a, w, src, pay)

    def _compiled(self, a, w, src, pay):
        """ReceptionistModel._compiled plus A_PUBLISH"""
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
                msg = ((v & 0xFFFFFF) | A.or_mask) if A.or_mask else (v & M32)
                x, bit = A.word & 1, 1 << (A.pad1 & 7)
                if A.op == typed.A_SET:
                    w[x] = v
                elif A.op == typed.A_ADD:
                    w[x] = (w[x] + v) & M64
                elif A.op == typed.A_MAX:
                    w[x] = max(w[x], v)
                elif A.op == typed.A_MIN:
                    w[x] = min(w[x], v)
                elif A.op == typed.A_REGISTER:
                    if not int(self.mask[a]) & bit:
                        self.mask[a] |= bit
                        self.info["registered"] += 1
                elif A.op == typed.A_DEREGISTER:
                    if int(self.mask[a]) & bit:
                        self.mask[a] &= ~bit & 0xFF
                        self.info["deregistered"] += 1
                elif A.op == typed.A_PUBLISH:
                    self.tinfo["published"] += 1
                    self._pubs.append((a, self._at[1], A.pad1 & 7, msg))
                elif A.op in (typed.A_TELL, typed.A_ROUTE):
                    d = 0
                    if A.op == typed.A_TELL or A.pad0 & typed.ROUTE_BY_INDEX:
                        if A.dsrc == typed.V_SELF and A.op == typed.A_TELL:
                            d = (a + A.dk) % self.n
                        else:
                            d = self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a)
                    ref = min(d, M32)
                    if A.op == typed.A_ROUTE:
                        L = self.listing[A.pad1 & 7]
                        if not L:
                            ref = NONE
                        elif A.pad0 & typed.ROUTE_BY_INDEX:
                            ref = L[d % len(L)]
                        else:
                            j = bisect_left(L, w[x])
                            ref = L[0 if j == len(L) else j]
                            w[x] = ref + 1
                        self.info["no_routees" if ref == NONE else "routed"] += 1
                    self._emit(src if A.pad0 & typed.ROUTE_KEEP_SENDER else a, ref, msg)
            if C.result == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME
            return C.result
        return UNHANDLED

    # ------------------------------------------------------------ supersteps
    def step(self) -> bool:
        if not self.log_cap:
            return super().step()
        deliveries, nosub = self._plan()
        if not (self.backlog or self.emitted_q or self.staged_q or deliveries):
            return False  # (no mail: no tick; a log without recipients waits)
        self.tinfo["fanned_out"] += len(deliveries)
        self.tinfo["no_subscribers"] += nosub
        self.tlog = []
        if deliveries:  # (a diagnostic of the tests: the deliveries a bounded mailbox refuses at admission)
            before, mine = {}, {}
            for d, _, _ in self.backlog + self.emitted_q + self.staged_q:
                before[d] = before.get(d, 0) + 1
            for d, _, _ in deliveries:
                mine[d] = mine.get(d, 0) + 1
            for d, k in mine.items():
                C = self._limits(d)[0]
                if C and self.alive[d]:
                    self.delivery_dead_letters += min(k, max(0, before.get(d, 0) + k - C))
        self.staged_q = self.staged_q + deliveries  # the inbox's tail, after the host-staged tells
        self._pubs, self._at = [], (None, 0)
        ok = super().step()
        assert ok
        self._pubs.sort(key=lambda e: (e[0], e[1]))
        if len(self._pubs) > self.log_cap:
            self.topic_error = True
            self._pubs = self._pubs[:self.log_cap]
        self.tlog = [(k, p, m) for p, _, k, m in self._pubs]
        self._pubs = []
        return True

    def run(self, max_supersteps: int = 1 << 30) -> dict:
        st = super().run(max_supersteps)
        planned, _ = self._plan()
        self.c["in_flight"] += len(planned)
        st["in_flight"] = self.c["in_flight"]
        return st
