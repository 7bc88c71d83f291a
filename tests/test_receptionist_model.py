"""The receptionist model (tests/receptionist_model.py) on the CPU: against the known answers
restated from the reference's specs (tests/golden/receptionist_kats.json), the documented round-robin difference,
the net-change version rule, and equality with PrioModel / the FIFO oracle where the registry is never touched."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from tests import receptionist_cases as rc
from tests.prio_model import PrioModel
from tests.receptionist_model import ReceptionistModel


def model_for(w):
    m = ReceptionistModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


@pytest.mark.parametrize("T", rc.KAT_T)
@pytest.mark.parametrize("name", rc.KAT_NAMES)
def test_kat(name, T):
    got = rc.run_kat(name, T, model_for(rc.kat_workload(name, T)))
    rc.check_kat(name, got)
    assert all(set(g) >= set(k for k in s if k not in ("tell", "route")) for s, g in zip(rc.SCENARIOS[name]["steps"], got))


def test_kats_cite_the_reference():
    assert len(rc.KAT_NAMES) == 14 and all("Spec.scala:" in s["cite"] for s in rc.KATS["scenarios"])


def test_round_robin_documented_difference():
    """DESIGN.md §2.8, bounded difference 1: listing [B, C], B picked, then A added.  The reference's one-step
    correction (RoutingLogic.scala:61-72) picks A next; the successor rule continues from where it was: C."""
    A, Bb, C = rc.IDS["A"], rc.IDS["B"], rc.IDS["C"]
    m = model_for(rc.node_workload(3, starts=[(Bb, 1, 0), (C, 1, 0)]))
    rc.tells(m, (rc.ROUTER, "Route:0"))
    m.run()
    rc.tells(m, (A, "Reg:0"))
    m.run()
    assert m.read_listing(0).tolist() == [A, Bb, C]
    rc.tells(m, (rc.ROUTER, "Route:1"))
    m.run()
    d, s, p = m.take_outbound()
    assert s.tolist() == [Bb, C]  # (the reference: [B, A])
    rc.tells(m, (rc.ROUTER, "Route:2"))  # ... and A's turn comes after the wrap
    m.run()
    assert m.take_outbound()[1].tolist() == [A]


def test_second_documented_example():
    """Listing [A..E], A-D picked, then A and B removed: the reference wraps to C, here the next pick is E."""
    ids = [rc.IDS[x] for x in "ABCDE"]
    m = model_for(rc.node_workload(1, starts=[(i, 1, 0) for i in ids]))
    rc.tells(m, *[(rc.ROUTER, f"Route:{i}") for i in range(4)])
    m.run()
    rc.tells(m, (ids[0], "Dereg:0"), (ids[1], "Dereg:0"))
    m.run()
    m.take_outbound()
    rc.tells(m, (rc.ROUTER, "Route:9"))
    m.run()
    assert m.take_outbound()[1].tolist() == [ids[4]]


@pytest.mark.parametrize("T", [1, 3])
def test_version_counts_net_changes(T):
    """Register and deregister in one window: nothing changes, no version moves, no rebuild is counted (T = 3);
    with T = 1 the two land in two ticks and the version moves twice."""
    A = rc.IDS["A"]
    m = model_for(rc.node_workload(T))
    rc.tells(m, (A, "Reg:0"), (A, "Dereg:0"))
    m.run()
    i = m.receptionist_info()
    assert (i["registered"], i["deregistered"]) == (1, 1) and m.read_listing(0).size == 0
    assert (i["version"][0], i["rebuilds"]) == ((0, 0) if T == 3 else (2, 2))
    rc.tells(m, (A, "Reg:1"), (A, "Reg:1"), (A + 1, "Reg:1"))  # idempotent; one version step for one tick's changes
    m.run(1)
    assert m.receptionist_info()["version"][1] == 1 and m.receptionist_info()["registered"] == 3


def test_visible_from_the_next_tick():
    """A change made while draining tick s is visible to every reader from tick s + 1, not within s."""
    A = rc.IDS["A"]
    m = model_for(rc.node_workload(3))
    rc.tells(m, (A, "Reg:0"), (A, "Size:0"))  # the same window: the size read is the listing in force
    m.run(1)
    assert [int(p) & 0xFFFFFF for p in m.take_outbound()[2]] == [0]
    rc.tells(m, (A, "Size:0"))
    m.run(1)
    assert [int(p) & 0xFFFFFF for p in m.take_outbound()[2]] == [1]


def test_no_routees_is_a_dead_letter_and_keeps_the_cursor():
    m = model_for(rc.node_workload(3))
    rc.tells(m, (rc.ROUTER, "Route:1"), (rc.ROUTER, "RouteBy:5"))
    st = m.run()
    assert (st["emitted"], st["dead_letters"]) == (2, 2) and m.receptionist_info()["no_routees"] == 2
    assert int(m.read_state()[0][rc.ROUTER, 0]) == 0
    assert st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def test_listing_capacity_error():
    m = model_for(rc.node_workload(3, listing_capacity=2))
    rc.tells(m, (1, "Reg:0"), (2, "Reg:0"))
    m.run()
    assert not m.capacity_error and m.read_listing(0).tolist() == [1, 2]
    rc.tells(m, (0, "Reg:0"))
    m.run()
    assert m.capacity_error and m.read_listing(0).tolist() == [0, 1]


@pytest.mark.parametrize("w", [wl.compiled(512, seed=3), wl.mixed(512, seed=4, capacity=4)], ids=lambda w: w.name)
def test_equals_prio_model_without_the_registry(w):
    """a workload that never touches the registry: the model is PrioModel, which tests/test_prio_model.py pins to the
    FIFO oracle"""
    w.max_emit = 1 if w.behaviors is None or w.behaviors.max_tells <= 1 else w.max_emit
    a, b = PrioModel(**w.engine_kwargs()), ReceptionistModel(**w.engine_kwargs())
    w.apply_to(a)
    w.apply_to(b)
    if b.kmax == 1:
        b.set_receptionist(2, 16)
    assert a.run() == b.run()
    assert np.array_equal(a.read_state()[0], b.read_state()[0]) and np.array_equal(a.read_state()[1], b.read_state()[1])
    assert b.receptionist_info()["rebuilds"] == 0


def test_service_mesh_model_runs_and_conserves():
    w = wl.service_mesh(512, ticks=12, seed=2)
    m = model_for(w)
    st = w.run_schedule(m)
    i = m.receptionist_info()
    assert st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]
    assert i["routed"] > 0 and i["terminated"] > 0 and i["deregistered"] > 0 and min(i["version"]) > 0
    assert m.max_bucket_inbox(64) <= 2048 and not m.capacity_error
    for k in range(8):
        assert m.read_listing(k).tolist() == np.flatnonzero((m.read_services() >> k) & 1).tolist()


def test_service_pool_listing_shrinks():
    w = wl.service_pool(8, 64, ticks=10, quota=3, n_host=2)
    m = model_for(w)
    sizes = []
    for dst, src, pay in w.schedule:
        m.tell(dst, pay, src)
        m.run(1)
        sizes.append(m.receptionist_info()["size"][0])
    m.run()
    assert sizes[0] == 64 and sizes[-1] < sizes[0] and sorted(sizes, reverse=True) == sizes
    assert m.receptionist_info()["terminated"] == 64 - m.receptionist_info()["size"][0]
    assert len(m.take_outbound()[0]) == m.receptionist_info()["routed"]  # every routed job answered its replyTo
