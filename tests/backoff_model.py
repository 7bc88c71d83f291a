"""A pure Python model of one dispatcher of the engine with restartWithBackoff: tests/supervision_model.
SupervisionModel plus DESIGN.md §2.14 (SupervisorStrategy.restartWithBackoff; the reference: TY/internal/
Supervision.scala:163-406 -- calculateDelay, aroundReceive, handleException, prepareRestart, restartCompleted,
updateRestartCount --, pinned by SupervisionSpec.scala:370-422 and :774-924).

  set_backoff(rows) comes after set_supervision, one row per (behaviour, level); a row with min_backoff != 0 turns
  the RESTART entry of that place into a backoff entry.  A failure caught by such an entry at tick t, the entry
  having the count c and the reset-due r (0: none; it lives in the entry's deadline word, which a backoff entry
  does not use otherwise) --
    1. r != 0 and t >= r: c := 0, r := none;
    2. max_restarts != -1 and c >= max_restarts: the actor stops (PostStop, stops++, limit_stops++); the failure
       does not pass to an outer entry;
    3. else PreRestart runs, c := c + 1, the inner entries are cleared, the kind becomes the initial kind, the
       reset words take their values, restarts++ and backoffs++;
    4. delay = c_before >= 30 ? max : min(max, min << c_before), plus (delay * q16 * r16) >> 32 with r16 the top
       16 bits of fanout_rand(seed, actor, t, 0);
    5. until := t + delay, r := until + reset_after (both saturate at 2^32 - 1).
  The window ends at the failing message.  While t < until nothing addressed to the actor is processed: the queue
  behind the failing message is cut to the stash capacity and held at the head of the backlog, later arrivals are
  admitted while the held length is below min(mailbox capacity, stash capacity); what is cut or refused is a dead
  letter and counts as dropped.  From tick `until` on the actor drains as always, the held mail first.

Without set_backoff, or with plain rows only, every result is SupervisionModel's.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from akka_amd import typed
from tests.prio_model import SAME, STOPPED, UNHANDLED, M32, fanout_rand
from tests.supervision_model import FAIL, SupervisionModel

SUSPENDED = -1   # _failed's third answer: the actor is restarted and backs off
BACKOFF_KEYS = ("backoffs", "resumed", "dropped", "limit_stops", "suspended")


@dataclass(frozen=True)
class BackoffRow:
    """include/akka_gpu.h agx_backoff"""
    min_backoff: int = 0
    max_backoff: int = 0
    random_factor_q16: int = 0
    reset_after: int = 1
    stash_capacity: int = -1


def calculate_delay(c: int, mn: int, mx: int) -> int:
    """calculateDelay (Supervision.scala:163-173) before the jitter: restartCount >= 30 -> max, else
    min(max, min * 2^restartCount)"""
    return mx if c >= 30 else min(mx, mn << c)


def jitter(delay: int, q16: int, r16: int) -> int:
    return (delay * q16 * r16) >> 32


def draw16(seed: int, actor: int, t: int) -> int:
    return fanout_rand(seed, actor, t & M32, 0) >> 48


class BackoffModel(SupervisionModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bo = None         # per compiled behaviour: its rows, inner first
        self.until = None      # [actor] the first tick at which the actor drains again (0: never suspended)
        self.cap = None        # [actor] the stash bound of its suspension (-1: none of its own)
        self.b = dict(backoffs=0, dropped=0, limit_stops=0)

    # ------------------------------------------------------------ setup
    def set_backoff(self, rows):
        assert self.rows is not None and self.bo is None and self.c["supersteps"] == 0
        rows = [list(r) for r in rows]
        assert len(rows) == len(self.rows)
        for sup, bo in zip(self.rows, rows):
            assert len(bo) <= self.n_levels
            for lev, r in enumerate(bo):
                if r.min_backoff == 0:
                    continue
                assert lev < len(sup) and sup[lev].class_mask and sup[lev].strategy == typed.SUP_RESTART
                assert 1 <= r.min_backoff <= r.max_backoff <= typed.MAX_TIMER_DELAY and r.reset_after >= 1
                assert 0 <= r.random_factor_q16 <= 65536 and r.stash_capacity >= -1
        self.bo = rows
        self.until = np.zeros(self.n, np.int64)
        self.cap = np.full(self.n, -1, np.int64)

    def _row(self, b, lev):
        if self.bo is None or not 0 <= b < len(self.bo) or lev >= len(self.bo[b]):
            return None
        r = self.bo[b][lev]
        return r if r.min_backoff else None

    # ------------------------------------------------------------ reading
    def backoff_info(self) -> dict:
        now = self.c["supersteps"]
        susp = 0 if self.until is None else int(np.count_nonzero(self.until > now + 1))
        return dict(self.b, resumed=self.b["backoffs"] - susp, suspended=susp)

    def read_backoff(self, a) -> dict:
        if self.until is None:
            return dict(suspended_for=0, until=0)
        u = int(self.until[a])
        return dict(suspended_for=max(u - 1 - self.c["supersteps"], 0), until=u)

    # ------------------------------------------------------------ the catch clause
    def _failed(self, a, w, res, cls, t) -> int:
        if self.bo is None or res != FAIL:
            return super()._failed(a, w, res, cls, t)
        ik = int(self.init_kind[a])
        b = ik - typed.KIND_COMPILED
        row = self.rows[b] if 0 <= b < len(self.rows) else []
        self.s["failures"] += 1
        for lev, E in enumerate(row):  # inner first
            if not (E.class_mask >> (cls & 31)) & 1:
                continue
            if E.strategy == typed.SUP_RESUME:
                self.s["resumes"] += 1
                return SAME
            if E.strategy != typed.SUP_RESTART:
                break
            R = self._row(b, lev)
            c, d = int(self.count[a, lev]), int(self.deadline[a, lev])
            if R is None:  # a plain restart: SupervisionModel's rule
                left = d == 0 or t <= d
                if E.max_restarts != -1 and c >= E.max_restarts and left:
                    continue  # rethrown (:316)
                self._signal(a, w, typed.SIGNAL_PRERESTART)
                self.count[a, lev] = c + 1 if left else 1
                self.deadline[a, lev] = d if (d != 0 and left) else t + E.within
            else:
                if d != 0 and t >= d:  # ResetRestartCount, lazily
                    c = d = 0
                    self.count[a, lev] = self.deadline[a, lev] = 0
                if E.max_restarts != -1 and c >= E.max_restarts:  # BehaviorImpl.failed: not rethrown (:314-320)
                    self.b["limit_stops"] += 1
                    break
                self._signal(a, w, typed.SIGNAL_PRERESTART)
                self.count[a, lev] = c + 1
                delay = calculate_delay(c, R.min_backoff, R.max_backoff)
                seed = self.fan[1] if self.fan else 0
                delay += jitter(delay, R.random_factor_q16, draw16(seed, a, t))
                until = min(t + delay, M32)
                self.until[a] = until
                self.deadline[a, lev] = min(until + R.reset_after, M32)
                C = self._limits(a)[0]
                self.cap[a] = R.stash_capacity if R.stash_capacity >= 0 else (C if C else -1)
                self.b["backoffs"] += 1
            self.count[a, :lev] = 0
            self.deadline[a, :lev] = 0
            self.kind[a] = ik
            for x in range(2):
                if (E.reset_mask >> x) & 1:
                    w[x] = int(E.reset[x])
            self.s["restarts"] += 1
            return SAME if R is None else SUSPENDED
        self._signal(a, w, typed.SIGNAL_POSTSTOP)
        self.s["stops"] += 1
        return STOPPED

    # ------------------------------------------------------------ supersteps
    def _cut(self, q, bound):
        """the first `bound` items are held (bound < 0: all); the rest are dead letters, dropped"""
        keep = len(q) if bound < 0 else min(len(q), bound)
        self.c["dead_letters"] += len(q) - keep
        self.b["dropped"] += len(q) - keep
        return q[:keep]

    def step(self) -> bool:
        if self.bo is None:
            return super().step()
        msgs = self.backlog + self.emitted_q + self.staged_q
        if not msgs:
            return False
        t = self.c["supersteps"] + 1  # this tick
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
            if t < self.until[a]:  # suspended: drain window 0, the admission bound is the stash bound
                S = int(self.cap[a])
                bound = S if C == 0 else (C if S < 0 else min(C, S))
                self.backlog += [(a, s, p) for s, p in self._cut(q, bound)]
                continue
            keep = L if C == 0 else min(L, C)
            self.c["dead_letters"] += L - keep
            adm = q[:keep]
            nd = min(keep, T)
            w = [int(self.words[a, 0]), int(self.words[a, 1])]
            rest = adm[nd:]
            for i in range(nd):
                sv, pv = adm[i]
                if int(self.kind[a]) >= typed.KIND_COMPILED:
                    r, cls = self._compiled_s(a, w, sv, pv, False)
                else:
                    r, cls = self._apply(a, w, sv, pv), 0
                self.c["delivered"] += 1
                if r == UNHANDLED:
                    self.c["unhandled"] += 1
                if r in (FAIL, STOPPED):
                    r = self._failed(a, w, r, cls, t)
                if r == SUSPENDED:  # the window ends here; what is queued behind stays queued, cut to the stash
                    rest = self._cut(adm[i + 1:], int(self.cap[a]))
                    break
                if r == STOPPED:
                    self.alive[a] = 0
                    self.c["dead_letters"] += nd - i - 1
                    break
            self.words[a, 0], self.words[a, 1] = w[0], w[1]
            self.backlog += [(a, s, p) for s, p in rest]
        self.emitted_q, self.staged_q = self._out, []
        self.inbox_sizes.append(sizes)
        self.c["supersteps"] += 1
        return True
