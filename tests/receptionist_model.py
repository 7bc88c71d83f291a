"""A pure Python model of an engine with the receptionist: PrioModel (the BSP superstep) plus
DESIGN.md §2.8 (the registry, the listings in force, find and route), in plain Python.

  * every actor holds one bit per service key; Register / Deregister set / clear the actor's own bit; a stop
    clears all of them (RegisteredActorTerminated, LocalReceptionist.scala:147-248);
  * the listing of key k in force during tick t is the ids whose bit was set at the end of tick t - 1, ascending;
    a change made while draining tick s is visible from tick s + 1;
  * version[k] grows by one at the end of every tick in which some actor's bit k differs from its value at the
    start of the tick (the net change over the tick); only such a key is rebuilt (`rebuilds`);
  * round robin: the smallest listed id >= the cursor, else listing[0]; the cursor becomes routee + 1; by index:
    listing[x mod size]; no routees: the message goes to 0xFFFFFFFF (emitted and a dead letter, `no_routees`),
    the cursor stays (GroupRouterImpl.scala:114-146, RoutingLogic.scala:42-75);
  * a forward keeps the incoming message's sender on the envelope.

Not fast; not meant to be."""
from __future__ import annotations

from bisect import bisect_left

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, STOPPED, UNHANDLED, PrioModel

NONE = 0xFFFFFFFF
INFO_KEYS = ("routed", "no_routees", "registered", "deregistered", "terminated", "rebuilds")


class ReceptionistModel(PrioModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n_keys = 0
        self.rcap = 0
        self.mask = np.zeros(self.n, np.uint8)
        self.listing = [[] for _ in range(8)]
        self.version = [0] * 8
        self.info = dict.fromkeys(INFO_KEYS, 0)
        self.capacity_error = False

    # ------------------------------------------------------------ the engine's calls
    def set_receptionist(self, n_keys, capacity):
        assert 1 <= n_keys <= 8 and capacity >= 1 and not self.n_keys
        assert self.kmax == 1, "a route must take effect once"
        self.n_keys, self.rcap = int(n_keys), min(int(capacity), self.n)

    def _rebuild(self, keys):
        for k in keys:
            ids = np.flatnonzero((self.mask >> k) & 1).tolist()
            if len(ids) > self.rcap:
                self.capacity_error = True
                ids = ids[:self.rcap]
            self.listing[k] = ids
            self.version[k] += 1
            self.info["rebuilds"] += 1

    def register_services(self, first, count, key, on=True):
        assert self.n_keys and key < self.n_keys
        bit, changed = 1 << key, False
        for a in range(first, first + count):
            if not self.alive[a] & 1:
                continue
            m = int(self.mask[a])
            m2 = m | bit if on else m & ~bit
            if m2 != m:
                self.mask[a] = m2
                self.info["registered" if on else "deregistered"] += 1
                changed = True
        if changed:
            self._rebuild([key])

    def read_listing(self, key):
        return np.asarray(self.listing[key], np.uint32)

    def read_services(self, first=0, count=None):
        count = self.n - first if count is None else count
        return self.mask[first:first + count].copy()

    def receptionist_info(self):
        d = dict(self.info)
        d["size"] = [len(x) for x in self.listing]
        d["version"] = list(self.version)
        return d

    def read_kinds(self):
        return self.kind.astype(np.uint8)

    # ------------------------------------------------------------ behaviours
    def _operand(self, src, word, k, pay, w, sender, self_id):
        if src == typed.V_LISTING_SIZE:
            return (len(self.listing[word & 7]) + k) & M64
        if src == typed.V_SERVICE_AT:
            sel = (word >> 3) & 3
            x = w[sel] if sel <= typed.SVC_WORD1 else (pay & 0xFFFFFF) if sel == typed.SVC_ARG else 0
            L = self.listing[word & 7]
            return L[((x + k) & M64) % len(L)] if L else NONE
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
        before = self.mask.copy()
        if not super().step():
            return False
        gone = np.flatnonzero((self.alive & 1) == 0)
        for a in gone.tolist():  # RegisteredActorTerminated: a stop of any cause clears the actor's bits
            if self.mask[a]:
                self.info["terminated"] += bin(int(self.mask[a])).count("1")
                self.mask[a] = 0
        diff = int(np.bitwise_or.reduce(before ^ self.mask)) if self.n else 0
        self._rebuild([k for k in range(8) if (diff >> k) & 1])
        return True
