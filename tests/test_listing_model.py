"""Subscribe / Find and the Listing message, without a GPU: the model of DESIGN.md §2.11 (tests/listing_model.py)
against the known answers restated from the reference's spec (tests/golden/listing_kats.json, LocalReceptionistSpec.scala
:81-175), each bounded difference of §2.11, and conservation after every run."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from tests import listing_cases as lc
from tests.listing_model import ListingModel


def model_for(w):
    m = ListingModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def play(w, script):
    """run the script on the model; conservation after every run; the last stats, snapshot and every report"""
    m = model_for(w)
    reports, st, snap = {}, None, None
    for st in script(m):
        st = lc.counts(st)
        snap = lc.snapshot(m)
        assert lc.conserved(st, snap["topic_info"], snap["listing_info"]), st
        for a, r in lc.reports_of(snap).items():
            reports.setdefault(a, []).extend(r)
    return st, snap, reports


def listings_of(reports, a):
    return [r[1:] for r in reports.get(a, []) if r[0] == "L"]


# ------------------------------------------------------------------ the known answers
@pytest.mark.parametrize("T", lc.KAT_T)
@pytest.mark.parametrize("name", lc.KAT_NAMES)
def test_kat(name, T):
    lc.check_kat(name, lc.run_kat(name, model_for(lc.node_workload(T))))


def test_kats_cite_the_spec():
    for s in lc.KATS["scenarios"]:
        assert s["cite"].startswith("LocalReceptionistSpec.scala:") and all("cite" in st for st in s["steps"])


# ------------------------------------------------------------------ the bounded differences
def test_coalescing_one_listing_per_key_and_tick():
    """difference 1: two registrations of one key in one tick, and two Finds of one key in one window, give one
    Listing, with the end-of-tick set"""
    def script(t):
        yield t.run()
        lc.tells(t, (6, "Reg:0"), (7, "Reg:0"), (22, "Find:1"), (22, "Find:1"))
        yield t.run()
    st, snap, rep = play(lc.node_workload(5, subscribed=[(10, 1, 0)]), script)
    assert listings_of(rep, 10) == [(0, 0), (0, 2)]
    assert listings_of(rep, 22) == [(1, 0)]
    assert snap["listing_info"] == dict(subscribes=1, finds=2, listings_sent=3, notified=1)


def test_initial_listing_exactly_one():
    """difference 2: a Subscribe in tick s gives exactly one Listing in s + 1, whether or not the key changed in s"""
    def script(t):
        lc.tells(t, (20, "Sub:0"), (6, "Reg:0"), (21, "Sub:1"))
        yield t.run()
    st, snap, rep = play(lc.node_workload(3), script)
    assert listings_of(rep, 20) == [(0, 1)] and listings_of(rep, 21) == [(1, 0)]
    assert snap["words"][20] == [1, 6] and snap["listing_info"]["notified"] == 1


def test_listings_are_ordered_by_key():
    """difference 3: key B changed and key A was found: A's Listing comes first"""
    def script(t):
        yield t.run()
        lc.tells(t, (6, "Reg:1"), (10, "Find:0"))
        yield t.run()
    st, snap, rep = play(lc.node_workload(3, subscribed=[(10, 1, 1)]), script)
    assert listings_of(rep, 10) == [(1, 0), (0, 0), (1, 1)]


def test_scope_one_rank_no_receptionist_actor():
    """difference 4: the Listing has no sender, and nobody but the subscriber receives anything"""
    m = model_for(lc.node_workload(3, subscribed=[(10, 1, 0)]))
    st = m.run(0)
    assert st["in_flight"] == 1 and [e for e in m.staged_q] == []
    out, _ = m._lplan()
    assert out == [(10, lc.NO_SENDER, lc.LISTING[0].payload(0))]


# ------------------------------------------------------------------ the rules
def test_timing_rules():
    st, snap, rep = play(lc.timing_workload(), lc.timing_script)
    assert listings_of(rep, 20) == [(0, 2), (0, 1), (0, 1)]   # subscribed with a change; 5's stop; the repeated Subscribe
    assert listings_of(rep, 21) == [(1, 0)]                   # subscribed without a change; (8's window moved nothing)
    assert listings_of(rep, 22) == [(0, 2)]                   # a Find is one shot
    assert listings_of(rep, 70) == [(0, 1), (0, 2), (0, 1)]   # the initial one; Find + change: one envelope; 5's stop
    assert listings_of(rep, 140) == [(0, 1), (0, 2)]          # stopped in the tick of the change: nothing more
    assert listings_of(rep, 23) == []                         # subscribe and stop in one window
    assert snap["sub"][140] == 0 and snap["pending"][140] == 0 and snap["sub"][23] == 0 and snap["pending"][23] == 0
    assert snap["alive"][23] == 0 and snap["sub"][20] == 1 and snap["info"]["version"][1] == 0


def test_stop_clears_both_masks():
    def script(t):
        lc.tells(t, (30, "Sub:0"), (30, "Find:1"), (30, "Stop"), (31, "Sub:1"))
        yield t.run(1)
        yield t.run()
    for T, dead in ((3, True), (1, False)):
        m = model_for(lc.node_workload(T))
        g = script(m)
        next(g)
        sub, pend = m.read_subscriptions()
        assert (int(sub[30]), int(pend[30])) == ((0, 0) if dead else (1, 1)) and (int(sub[31]), int(pend[31])) == (2, 2)
        next(g)
        sub, pend = m.read_subscriptions()
        assert int(sub[30]) == 0 and int(pend[30]) == 0 and not m.alive[30] & 1


def test_bounded_mailbox_gives_a_dead_letter():
    st, snap, rep = play(lc.bounded_workload(), lc.bounded_script)
    assert st["dead_letters"] == 128 and snap["listing_info"]["listings_sent"] == 4 * 128
    assert listings_of(rep, 64) == [(0, 0), (1, 1), (0, 1)]  # (B's first Listing waited: it sees the newer set)


def test_budgets():
    m = model_for(lc.order_workload())
    assert m.run(1)["in_flight"] == 0 and m.run()["supersteps"] == 1  # (the initial Listings)
    lc.tells(m, (7, "Reg:0"))
    st = m.run(1)
    assert st["in_flight"] == 7 and m.listing_info()["listings_sent"] == 10 + 7  # owed, not yet drained
    st = m.run()
    assert st["in_flight"] == 0 and st["supersteps"] == 3
    assert m.run()["supersteps"] == 3
    play(lc.order_workload(), lc.budget_script)


def test_order_and_host_calls():
    st, snap, rep = play(lc.order_workload(), lc.order_script)
    assert rep[64] == [("L", 0, 1), ("L", 1, 1), ("G", 64), ("G", 8), ("G", 9), ("L", 0, 2), ("L", 1, 0)]
    st, snap, rep = play(lc.order_workload(1), lc.backlog_script)
    # (queued behind the Pings: both Listings see the listing in force when they are drained)
    assert rep[64][-5:] == [("G", 1), ("G", 2), ("G", 3), ("L", 0, 3), ("L", 0, 3)]
    st, snap, rep = play(lc.order_workload(), lc.host_calls_script)
    assert listings_of(rep, 100) == [(0, 1), (0, 3), (0, 5), (0, 7)] and listings_of(rep, 63)[:3] == [(0, 1), (1, 1), (1, 2)]
    assert listings_of(rep, 64) == [(0, 1), (1, 1), (0, 3), (0, 5), (0, 7), (1, 2), (1, 3)]


@pytest.mark.parametrize("seed", lc.MESH_SEEDS)
def test_mesh_conserves(seed):
    w = lc.mesh_workload(seed, 256, 64)
    st, snap, rep = play(w, lc.mesh_script(w))
    li = snap["listing_info"]
    assert li["listings_sent"] > li["subscribes"] and li["notified"] > 0 and st["dead_letters"] > 0


def test_workloads():
    w = wl.service_watchers(4, 32, ticks=6)
    st, snap, rep = play(w, lc.mesh_script(w))
    assert snap["listing_info"] == dict(subscribes=32, finds=0, listings_sent=7 * 32, notified=6)
    assert snap["words"][-1] == [7, 2]  # seven Listings; four services, and the two of the last two ticks are away
    w = wl.discovery_workers(4, 16, jobs=4)
    st, snap, rep = play(w, lc.mesh_script(w))
    assert [x[0] for x in snap["words"][:4]] == [16] * 4 and snap["listing_info"]["finds"] == 16 * 5
