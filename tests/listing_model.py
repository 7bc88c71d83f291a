"""A pure Python model of an engine with Receptionist.Subscribe / Find and the Listing message: TopicModel (DESIGN.md
§2.10) plus DESIGN.md §2.11, in plain Python.

  * every actor holds two more masks: `sub` (bit k: subscribed to key k) and `pending` (bit k: one Listing of key k
    is owed at the next tick); A_SUBSCRIBE_LISTING sets both of the actor's own bits (also when repeated), A_FIND the
    pending bit only; a stop of any cause clears both masks;
  * key k changed in tick s exactly when version[k] moved at the end of tick s (the receptionist's rebuild), or when
    register_services changed a bit between two runs;
  * when the inbox of tick s + 1 is formed, an alive actor receives one Listing(k) -- sender NO_SENDER, payload
    listing_payload[k] -- if its pending bit k is set, or if k changed and its sub bit k is set: one envelope per
    (actor, key); the pending bits served are cleared, and so is the set of changed keys;
  * the Listings are the inbox's tail after the publications, in ascending key and per key ascending id; admission
    is by position as for any mail;
  * owed Listings are in flight: staged + emitted + fanned_out + listings_sent = delivered + dead_letters + in_flight;
  * a tick is a superstep with mail: changed keys without a recipient wait for the next tick.

Not fast; not meant to be."""
from __future__ import annotations

from bisect import bisect_left

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, UNHANDLED
from tests.receptionist_model import NONE, ReceptionistModel
from tests.topic_model import NO_SENDER, TopicModel

LISTING_INFO_KEYS = ("subscribes", "finds", "listings_sent", "notified")


class ListingModel(TopicModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lpay = None                          # listing_payload[k]
        self.sub = np.zeros(self.n, np.uint8)
        self.pend = np.zeros(self.n, np.uint8)
        self.changed = 0                          # bit k: the next tick's Listings announce a change of key k
        self.linfo = dict.fromkeys(LISTING_INFO_KEYS, 0)  # (listings_sent / notified: of the ticks formed so far)

    # ------------------------------------------------------------ the engine's calls
    def set_listings(self, payloads):
        assert self.log_cap, "listings need topics"
        assert self.lpay is None and len(payloads) == self.n_keys
        self.lpay = [int(p) & M32 for p in payloads]

    def subscribe_listings(self, first, count, key, on=True):
        assert self.lpay is not None and key < self.n_keys
        bit = 1 << key
        for a in range(first, first + count):
            if not self.alive[a] & 1:
                continue
            s, p = int(self.sub[a]), int(self.pend[a])
            s2, p2 = (s | bit, p | bit) if on else (s & ~bit, p)
            if on and (s2, p2) != (s, p):
                self.linfo["subscribes"] += 1
            self.sub[a], self.pend[a] = s2, p2

    def read_subscriptions(self, first=0, count=None):
        count = self.n - first if count is None else count
        return self.sub[first:first + count].copy(), self.pend[first:first + count].copy()

    def _rebuild(self, keys):
        keys = list(keys)
        super()._rebuild(keys)
        if self.lpay is not None:
            for k in keys:
                self.changed |= 1 << k

    def _lplan(self):
        """the Listings owed against the masks as they are now, and the changed keys that have a recipient"""
        out, ntf = [], 0
        if self.lpay is None:
            return out, ntf
        for k in range(self.n_keys):
            chg = (self.changed >> k) & 1
            m = self.pend | (self.sub if chg else 0)
            ids = np.flatnonzero((m >> k) & 1).tolist()
            ntf += bool(chg and ids)
            out += [(a, NO_SENDER, self.lpay[k]) for a in ids]
        return out, ntf

    def listing_info(self):
        d = dict(self.linfo)
        planned, ntf = self._lplan()
        d["listings_sent"] += len(planned)
        d["notified"] += ntf
        return d

    # ------------------------------------------------------------ behaviours
    def _compiled(self, a, w, src, pay):
        """TopicModel._compiled plus A_SUBSCRIBE_LISTING / A_FIND"""
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
                elif A.op == typed.A_SUBSCRIBE_LISTING:
                    self.sub[a] |= bit
                    self.pend[a] |= bit
                    self.linfo["subscribes"] += 1
                elif A.op == typed.A_FIND:
                    self.pend[a] |= bit
                    self.linfo["finds"] += 1
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
        if self.lpay is None:
            return super().step()
        deliveries, nosub = self._plan()
        listings, ntf = self._lplan()
        if not (self.backlog or self.emitted_q or self.staged_q or deliveries or listings):
            return False  # (no mail: no tick; a log or a change without recipients waits)
        self.tinfo["fanned_out"] += len(deliveries)
        self.tinfo["no_subscribers"] += nosub
        self.tlog = []
        self.linfo["listings_sent"] += len(listings)
        self.linfo["notified"] += ntf
        self.changed = 0
        self.pend[:] = 0
        self.staged_q = self.staged_q + deliveries + listings  # the inbox's tail, after the host-staged tells
        self._pubs, self._at = [], (None, 0)
        ok = ReceptionistModel.step(self)
        assert ok
        gone = (self.alive & 1) == 0  # a stop of any cause clears both masks
        self.sub[gone] = 0
        self.pend[gone] = 0
        self._pubs.sort(key=lambda e: (e[0], e[1]))
        if len(self._pubs) > self.log_cap:
            self.topic_error = True
            self._pubs = self._pubs[:self.log_cap]
        self.tlog = [(k, p, m) for p, _, k, m in self._pubs]
        self._pubs = []
        return True

    def run(self, max_supersteps: int = 1 << 30) -> dict:
        st = super().run(max_supersteps)
        planned, _ = self._lplan()
        self.c["in_flight"] += len(planned)
        st["in_flight"] = self.c["in_flight"]
        return st
