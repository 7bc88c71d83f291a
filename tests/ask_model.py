"""A pure Python model of one dispatcher of the engine with the ask pattern: the timers' model (tests/timer_model.py,
DESIGN.md §2.3) plus §2.9 (ActorContext.ask: TY/internal/ActorContextImpl.scala:203-218; AskPattern.ask:
TY/scaladsl/AskPattern.scala:109-162; pinned by ActorContextAskSpec.scala:41-189 and AskSpec.scala:64-110).

  an outstanding ask is a single timer slot marked as an ask (with an adapt tag or none);
  ask of key k at tick s: the key is started as a single timer (cancel, next generation g, next fire s + delay, the
    stored payload is the timeout message), marked, and one envelope goes to the target whose sender field is the
    ask ref  1<<31 | k<<29 | (g mod 2^7)<<22 | the asker's id;
  answering: every tell whose destination has bit 31 set and is not 0xFFFFFFFF is a reply -- emitted to the ref's
    id with the ref as the sender field;
  receipt: a drained envelope whose sender field is a ref naming the receiver is a reply: delivered; slot k active,
    an ask, the same generation mod 2^7 -> the slot becomes inactive (a cancel), `answered`, the behaviour runs with
    sender = self on the adapted payload; else `late`, the behaviour does not run;
  timeout: the slot's TimerMsg accepted on an ask slot -> `timed_out`, the behaviour runs on the stored message.

It takes the same calls as GpuEngine, so with nothing asked it is the timers' model."""
from __future__ import annotations

import numpy as np

from akka_amd import typed
from tests.prio_model import BECOME, M32, M64, SAME, STOPPED, UNHANDLED
from tests.timer_model import GEN_MASK, NONE, TAG_TIMER, TimerModel, clamp_delay

REF_BIT, KEY_SHIFT, GEN_SHIFT, REF_GEN_MASK, ID_MASK = 1 << 31, 29, 22, 0x7F, (1 << 22) - 1
NO_ADAPT = 0xFFFFFFFF


def ask_ref(key: int, gen: int, actor: int) -> int:
    return REF_BIT | (key << KEY_SHIFT) | ((gen & REF_GEN_MASK) << GEN_SHIFT) | actor


def is_ref(x: int) -> bool:
    return bool(x & REF_BIT) and x != M32


class AskModel(TimerModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ask_on = False
        self.marks = None  # [actor][key]: None (no ask's timeout) or (adapt tag or None,)
        self.a = dict(asked=0, answered=0, timed_out=0, late=0)
        self._ref = 0      # the ref the running case's ARM left for its SEND

    # ------------------------------------------------------------ setup
    def set_ask(self):
        assert self.n_keys and not self.ask_on, "on top of the timers, once"
        assert self.n <= ID_MASK, "an ask ref carries the asker's id in 22 bits"
        self.ask_on = True
        self.marks = [[None] * self.n_keys for _ in range(self.n)]

    def _start(self, a, key, periodic, delay, payload, period=None):
        super()._start(a, key, periodic, delay, payload, period)
        if self.ask_on:
            self.marks[a][key] = None  # (a plain timer: the ARM marks the slot after its start)

    def tell(self, dst, payload, src=None):
        if self.ask_on and src is not None:
            s = np.atleast_1d(np.asarray(src, np.uint32))
            assert not np.any((s >> 31 != 0) & (s != M32)), "a host tell's sender is an actor id"
        super().tell(dst, payload, src)

    # ------------------------------------------------------------ reading
    def ask_info(self) -> dict:
        return dict(self.a)

    def read_asks(self, a) -> dict:
        o = dict(is_ask=np.zeros(4, np.uint32), adapt=np.full(4, NO_ADAPT, np.uint32))
        if self.ask_on:
            for k in range(self.n_keys):
                m = self.marks[a][k]
                if self.slots[a][k].active and m is not None:
                    o["is_ask"][k] = 1
                    o["adapt"][k] = NO_ADAPT if m[0] is None else m[0]
        return o

    # ------------------------------------------------------------ behaviours
    def _emit(self, self_id, dst, pay):
        dst &= M32
        if self.ask_on and is_ref(dst):  # the reply: to the ref's id, the ref as the sender field
            return super()._emit(dst, dst & ID_MASK, pay)
        return super()._emit(self_id, dst, pay)

    def _compiled(self, a, w, src, pay):
        if not self.ask_on:
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
                elif A.op in (typed.A_TELL, typed.A_ASK_SEND):
                    if A.dsrc == typed.V_SELF:
                        d = (a + A.dk) % self.n
                    else:
                        d = self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a)
                    if A.op == typed.A_TELL:
                        self._emit(a, min(d, M32), msg)
                    else:  # the ask's one envelope: the ref instead of the asker's id, and no reply rewrite
                        TimerModel._emit(self, self._ref, min(d, M32), msg)
                elif A.op in (typed.A_TIMER_SINGLE, typed.A_TIMER_PERIODIC):
                    d = clamp_delay(self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a))
                    self._cancel(a, A.word)
                    self._start(a, A.word, A.op == typed.A_TIMER_PERIODIC, d, msg)
                elif A.op == typed.A_TIMER_CANCEL:
                    self._cancel(a, A.word)
                elif A.op == typed.A_TIMER_CANCEL_ALL:
                    for k in range(self.n_keys):
                        self._cancel(a, k)
                elif A.op == typed.A_ASK_ARM:
                    d = clamp_delay(self._operand(A.dsrc, A.dword, A.dk, pay, w, src, a))
                    self._cancel(a, A.word)
                    self._start(a, A.word, False, d, msg)
                    self.marks[a][A.word] = (A.pad1 if A.pad0 & 1 else None,)
                    self._ref = ask_ref(A.word, self.slots[a][A.word].gen, a)
                    self.a["asked"] += 1
            if C.result == BECOME:
                self.kind[a] = typed.KIND_COMPILED + C.next
                return SAME
            return C.result
        return UNHANDLED

    # ------------------------------------------------------------ supersteps
    def step(self) -> bool:
        if not self.ask_on:
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
                        self.a["timed_out"] += self.marks[a][key] is not None  # an ask's timeout
                    sv, pv = a, s.payload
                elif is_ref(sv) and sv & ID_MASK == a:  # a reply
                    key = (sv >> KEY_SHIFT) & 3
                    s = self.slots[a][key] if key < self.n_keys else None
                    m = self.marks[a][key] if key < self.n_keys else None
                    if s is None or not s.active or m is None or (s.gen ^ (sv >> GEN_SHIFT)) & REF_GEN_MASK:
                        self.a["late"] += 1
                        continue
                    self._cancel(a, key)
                    self.a["answered"] += 1
                    sv = a
                    if m[0] is not None:
                        pv = (pv & 0xFFFFFF) | (m[0] << 24)
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
