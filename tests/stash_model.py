"""A pure Python model of one dispatcher of the engine with deque-based mailboxes: DESIGN.md §2 (the BSP
superstep, tests/prio_model.py) plus §2.2 (the stash) restated.

Every actor of a mailbox class with a stash capacity S has, outside its mailbox, a buffer B (at most S
envelopes, its first `rel` released) and a park P.  A superstep of such an actor takes its drain window
from one source -- the first min(rel, T) of B, else the first min(|P|, T) of P, else the first
min(keep, T) admitted mailbox messages; with B or P as the source every admitted mailbox message is
queued.  Each window message is removed from its source and processed: `stash` appends it to B (a full
B stops the actor), `unstash_all` releases what B holds, ends the drain and -- from the mailbox --
parks the unprocessed rest of the window.  A stop turns the rest of the window, B and P into dead
letters.  (StashBufferImpl.scala:61-79,131-218.)
"""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M64, SAME, STOPPED, UNHANDLED, PrioModel

STASH, UNSTASH_ALL = typed.RES_STASH, typed.RES_UNSTASH_ALL


class StashModel(PrioModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.scap = {}                 # class -> stash capacity
        self.B = {}                    # actor -> [(src, payload)]
        self.rel = {}                  # actor -> released entries at the head of B
        self.P = {}                    # actor -> parked [(src, payload)]
        self.sc = dict(stashed=0, unstashed=0, overflows=0)
        self._size = 0
        self.trace = []                # per superstep: what the guards of the GPU scenarios look at

    # ------------------------------------------------------------ setup / inspection
    def set_stash(self, cls, capacity):
        assert self.mcap[cls] is not None, "class not configured"
        assert 1 <= capacity <= 255
        self.scap[cls] = int(capacity)

    def stash_info(self):
        held = sum(len(b) - self.rel.get(a, 0) for a, b in self.B.items())
        pend = sum(self.rel.values()) + sum(len(p) for p in self.P.values())
        return dict(self.sc, held=held, pending=pend)

    def read_kinds(self):
        return self.kind.astype(np.uint8)

    def read_stash(self, a, cap=255):
        b = self.B.get(a, [])[:cap]
        return (np.asarray([s for s, _ in b], np.uint32), np.asarray([p for _, p in b], np.uint32), self.rel.get(a, 0))

    # ------------------------------------------------------------ behaviours
    def _operand(self, src, word, k, pay, w, sender, self_id):
        if src == typed.V_STASH:
            return (self._size + k) & M64
        return super()._operand(src, word, k, pay, w, sender, self_id)

    def _compiled(self, a, w, src, pay):
        t = self.tables
        b = int(self.kind[a]) - typed.KIND_COMPILED
        if t is not None and b < t.n_behaviors:
            # the first matching case decides; an unstash_all's become is applied here (PrioModel knows BECOME only)
            for ci in range(int(t.first[b]), int(t.first[b + 1])):
                C = t.cases[ci]
                if self._cmp(C.cmp1, self._operand(C.src1, C.word1, C.k1, pay, w, src, a),
                             self._operand(C.src2, C.word2, C.k2, pay, w, src, a)) and \
                   self._cmp(C.cmp2, self._operand(C.src3, C.word3, C.k3, pay, w, src, a),
                             self._operand(C.src4, C.word4, C.k4, pay, w, src, a)):
                    r = super()._compiled(a, w, src, pay)   # (runs that same case: tests read w before its actions)
                    if C.result == UNSTASH_ALL and C.next != typed.NEXT_SAME:
                        self.kind[a] = typed.KIND_COMPILED + C.next
                    return r
        return super()._compiled(a, w, src, pay)

    # ------------------------------------------------------------ supersteps
    def _cap(self, a):
        return self.scap.get(int(self.mcls[a]), 0)

    def step(self) -> bool:
        msgs = self.backlog + self.emitted_q + self.staged_q
        pending = {a for a, r in self.rel.items() if r > 0} | {a for a, p in self.P.items() if p}
        if not msgs and not pending:
            return False
        inbox = {}
        for d, s, p in msgs:
            inbox.setdefault(d, []).append((s, p))
        sizes = np.zeros(self.n, np.int64)
        self.backlog, self._out = [], []
        tr = dict(pending_no_mail=sorted(a for a in pending if a not in inbox), mail=sorted(inbox), park_left=0)
        for a in sorted(set(inbox) | pending):
            q = inbox.get(a, [])
            L = len(q)
            sizes[a] = L
            if not self.alive[a]:
                self.c["dead_letters"] += L
                continue
            C, T = self._limits(a)
            keep = L if C == 0 else min(L, C)
            self.c["dead_letters"] += L - keep
            adm = q[:keep]
            B, P = self.B.setdefault(a, []), self.P.setdefault(a, [])
            rel, S = self.rel.get(a, 0), self._cap(a)
            if rel > 0:
                source, window, queued = "B", B[:min(rel, T)], adm
            elif P:
                source, window, queued = "P", P[:min(len(P), T)], adm
            else:
                source, window, queued = "I", adm[:min(keep, T)], adm[min(keep, T):]
            if source != "I":
                sizes[a] += len(window)          # (the window shares the bucket's tile on the device)
            w = [int(self.words[a, 0]), int(self.words[a, 1])]
            i = 0
            while i < len(window):
                s, p = window[i]
                i += 1
                if source == "B":
                    B.pop(0)
                    rel -= 1
                elif source == "P":
                    P.pop(0)
                self._size = len(B)
                r = self._apply(a, w, s, p)
                if r == STASH:
                    if len(B) >= S:              # StashOverflowException: the actor fails and stops
                        r = STOPPED
                        self.sc["overflows"] += 1
                    else:
                        B.append((s, p))
                        self.sc["stashed"] += 1
                if r != STASH:
                    self.c["delivered"] += 1
                if r == UNHANDLED:
                    self.c["unhandled"] += 1
                if r == STOPPED:
                    self.alive[a] = 0
                    rest = len(window) - i if source == "I" else 0
                    self.c["dead_letters"] += rest + len(B) + len(P)
                    B.clear()
                    P.clear()
                    rel = 0
                    break
                if r == UNSTASH_ALL and B:
                    self.sc["unstashed"] += len(B) - rel
                    rel = len(B)
                    if source == "I":
                        P.extend(window[i:])
                        tr["park_left"] += 1 if window[i:] else 0
                    break
            self.rel[a] = rel
            self.words[a, 0], self.words[a, 1] = w[0], w[1]
            self.backlog += [(a, s, p) for s, p in queued]
        self.emitted_q, self.staged_q = self._out, []
        self.inbox_sizes.append(sizes)
        self.trace.append(tr)
        self.c["supersteps"] += 1
        return True

    def run(self, max_supersteps: int = 1 << 30) -> dict:
        st = super().run(max_supersteps)
        st["in_flight"] += sum(len(b) for b in self.B.values()) + sum(len(p) for p in self.P.values())
        self.c["in_flight"] = st["in_flight"]
        return st
