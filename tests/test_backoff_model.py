"""tests/backoff_model.py against the known answers worked out from the reference's SupervisionSpec
(tests/golden/backoff_kats.json), the delay table, the reset's exact tick, and SupervisionModel where no row backs
off.  No GPU."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd import workloads as wl
from tests import backoff_cases as bc
from tests import supervision_cases as sc
from tests.backoff_model import BackoffModel, BackoffRow, calculate_delay, draw16, jitter
from tests.supervision_model import SupervisionModel


def model_for(w, cls=BackoffModel):
    m = cls(**w.engine_kwargs())
    w.apply_to(m)
    return m


@pytest.mark.parametrize("T", bc.KAT_T)
@pytest.mark.parametrize("name", bc.KAT_NAMES)
def test_kat(name, T):
    got = bc.run_kat(name, T, model_for(bc.kat_workload(name, T)))
    bc.check_kat(name, T, got)


def test_every_kat_cites_its_spec_lines():
    for s in bc.KATS["scenarios"]:
        lo, hi = (int(x) for x in s["spec"].split("-"))
        assert 370 <= lo < hi <= 924, s["name"]
    assert len(bc.KAT_NAMES) == 6


# ------------------------------------------------------------------ the delay
def test_delay_table():
    """calculateDelay (Supervision.scala:163-173) for the counts 0..31: doubling, the clamp, >= 30 -> max"""
    mn, mx = 3, 1000
    want = [3, 6, 12, 24, 48, 96, 192, 384, 768] + [1000] * 23
    assert [calculate_delay(c, mn, mx) for c in range(32)] == want
    big = typed.MAX_TIMER_DELAY
    assert [calculate_delay(c, 1, big) for c in (0, 29, 30, 31)] == [1, 1 << 29, big, big]   # (2^29 < max: no clamp yet)
    assert calculate_delay(29, 5, big) == big and calculate_delay(30, 1, 7) == 7 and calculate_delay(0, 9, 9) == 9


@pytest.mark.parametrize("q16", [0, 13107, 65536])
def test_jitter_bounds(q16):
    """the jitter lies in [0, delay * q16 / 65536), comes after the clamp and may pass max; 64-bit integers only"""
    for delay in (1, 7, 1000, typed.MAX_TIMER_DELAY):
        assert jitter(delay, q16, 0) == 0
        top = jitter(delay, q16, 65535)
        assert top == (delay * q16 * 65535) >> 32 and top <= delay * q16 // 65536 and top < (1 << 31)
        assert delay * q16 * 65535 < (1 << 64)
        if q16 == 65536 and delay >= 65536:
            assert top > 0 and delay + top > delay            # (past the clamp)
    draws = [draw16(7, a, t) for a in range(64) for t in range(1, 9)]
    assert all(0 <= r < 65536 for r in draws) and len(set(draws)) > 400
    assert draw16(7, 3, 5) == draw16(7, 3, 5) != draw16(8, 3, 5)


def jitter_workload(q16, seed):
    w = bc.mix_workload(64, 3, (("E1", bc.backoff(1000, 1000, q16, reset_after=1)),))
    w.fanout = (1, seed, np.asarray([0xFFFFFFFF], np.uint32), np.asarray([0], np.uint32))
    return w


@pytest.mark.parametrize("q16", [0, 13107, 65536])
def test_jitter_in_the_model(q16):
    """`until` of 64 actors failing at tick 1: t + delay + jitter, the draw keyed by the seed, the actor and the tick"""
    m = model_for(jitter_workload(q16, 99))
    bc.tells(m, *[(a, bc.MIX_THROW, bc.E1) for a in range(64)])
    m.run(1)
    until = [m.read_backoff(a)["until"] for a in range(64)]
    assert until == [1 + 1000 + ((1000 * q16 * draw16(99, a, 1)) >> 32) for a in range(64)]
    assert all(1001 <= u <= 1001 + 1000 * q16 // 65536 for u in until)
    assert (len(set(until)) == 1) == (q16 == 0)


# ------------------------------------------------------------------ the reset
@pytest.mark.parametrize("gap, count", [(-1, 2), (0, 1)])
def test_reset_exactly_at_until_plus_reset_after(gap, count):
    """min 2, reset_after 5: a failure at tick 1 gives until 3 and reset-due 8.  A second failure one tick before the
    reset-due doubles the delay (count 2); one at the reset-due itself starts from the minimum again (count 1)"""
    m = model_for(bc.mix_workload(64, 3, (("E1", bc.backoff(2, 64, reset_after=5)),)))
    bc.tells(m, (40, bc.MIX_THROW, bc.E1))
    bc.mix_tick(m, 8 + gap - 1, (16, 17))
    m.run()
    assert m.c["supersteps"] == 8 + gap - 1 and m.read_backoff(40)["until"] == 3
    assert m.read_supervision(40)["remaining"][0] == 8 - m.c["supersteps"]
    bc.tells(m, (40, bc.MIX_THROW, bc.E1))
    m.run(1)
    t = 8 + gap
    assert m.read_supervision(40)["count"][0] == count
    assert m.read_backoff(40)["until"] == t + (4 if count == 2 else 2)
    assert m.read_supervision(40)["remaining"][0] == (4 if count == 2 else 2) + 5


# ------------------------------------------------------------------ plain rows
@pytest.mark.parametrize("n", [96, 70])
def test_plain_rows_give_the_supervision_models_results(n):
    w = sc.mix_workload(n, 3)
    a, b = model_for(w, SupervisionModel), model_for(w, BackoffModel)
    b.set_backoff([[BackoffRow()] for _ in w.supervision["rows"]])
    for sa, sb in zip(sc.shapes_script(n)(a), sc.shapes_script(n)(b)):
        assert sa == sb and sc.snapshot(a, range(n)) == sc.snapshot(b, range(n))
    assert b.backoff_info() == dict(backoffs=0, resumed=0, dropped=0, limit_stops=0, suspended=0)
    c = model_for(wl.flaky_workers(512, bucket_actors=64), BackoffModel)   # (never set: SupervisionModel's step)
    d = model_for(wl.flaky_workers(512, bucket_actors=64), SupervisionModel)
    assert c.run() == d.run() and c.supervision_info() == d.supervision_info()


# ------------------------------------------------------------------ held mail, the stash bound, conservation
def test_held_mail_keeps_its_order_and_the_bound_cuts_the_tail():
    m = model_for(bc.mix_workload(64, 2, (("E1", bc.backoff(4, 4, stash=3)),)))
    bc.tells(m, (40, bc.MIX_THROW, bc.E1), *[(40, bc.MIX_INC, i) for i in range(1, 6)])
    st = m.run()
    assert m.backoff_info() == dict(backoffs=1, resumed=1, dropped=2, limit_stops=0, suspended=0)
    assert st["dead_letters"] == 2 and st["supersteps"] == 6 and m.words[40].tolist() == [3, (bc.MIX_INC << 24) | 3]
    assert st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


@pytest.mark.parametrize("name", ["backoff_workers", "backoff_stash_pressure"])
def test_workloads_conserve_and_recover(name):
    w = wl.backoff_workers(1 << 10) if name == "backoff_workers" else wl.backoff_stash_pressure(1 << 10)
    m = model_for(w)
    st = m.run()
    assert st["in_flight"] == 0 and st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"]
    info = m.backoff_info()
    # (a target whose stash dropped everything stays suspended at the end: time does not pass without mail)
    assert info["backoffs"] > 50 and info["resumed"] + info["suspended"] == info["backoffs"]
    assert info["suspended"] == (0 if name == "backoff_workers" else int(np.count_nonzero(m.until > st["supersteps"] + 1)))
    assert m.max_bucket_inbox(w.bucket_actors) <= 2048
    if name == "backoff_workers":
        assert int(m.count.max()) > 3 and st["dead_letters"] == 0    # the counts pass 3; nothing is lost
    else:
        assert info["dropped"] > 50 and info["dropped"] <= st["dead_letters"]
