"""The priority and control-aware mailbox types of the dispatch layer (akka_amd/dispatch.py;
Mailbox.scala:726-816, 867-1025), host side: HOCON lookup, the registry that stands in for the user's
subclass of the abstract priority types, the tables they hand to the engine, and the refusals."""
import pytest

from akka_amd.config import Config, ConfigurationException
from akka_amd.dispatch import (BoundedControlAwareMailbox, BoundedPriorityMailbox, BoundedStablePriorityMailbox,
                               Mailboxes, UnboundedControlAwareMailbox, UnboundedPriorityMailbox,
                               UnboundedStablePriorityMailbox, priority_table)

CONF = Config.parse_string("""
ctl-unbounded {
  mailbox-type = "akka.dispatch.UnboundedControlAwareMailbox"
  gpu.control-tags = [3, 200]
}
ctl-bounded {
  mailbox-type = "akka.dispatch.BoundedControlAwareMailbox"
  mailbox-capacity = 16
  mailbox-push-timeout-time = 0s
  gpu.control-tags = [9]
}
ctl-blocking {
  mailbox-type = "akka.dispatch.BoundedControlAwareMailbox"
  mailbox-capacity = 16
  mailbox-push-timeout-time = 10s
}
my-prio {
  mailbox-type = "com.example.MyPriorityMailbox"
  mailbox-capacity = 1000
  mailbox-push-timeout-time = 0s
}
my-prio-blocking {
  mailbox-type = "com.example.MyPriorityMailbox"
  mailbox-capacity = 1000
  mailbox-push-timeout-time = 10s
}
unknown-prio {
  mailbox-type = "com.example.NotRegistered"
}
""")


def test_control_aware_lookup():
    mbs = Mailboxes(CONF)
    u = mbs.lookup("ctl-unbounded")
    assert isinstance(u, UnboundedControlAwareMailbox) and u.capacity == 0 and u.control_tags == (3, 200)
    assert u.priority_table == bytes(0 if t in (3, 200) else 1 for t in range(256))
    b = mbs.lookup("ctl-bounded")
    assert isinstance(b, BoundedControlAwareMailbox) and b.capacity == 16
    assert b.priority_table == bytes(0 if t == 9 else 1 for t in range(256))
    with pytest.raises(ConfigurationException, match="push"):
        mbs.lookup("ctl-blocking")


def test_control_aware_without_tags_is_one_queue():
    assert UnboundedControlAwareMailbox().priority_table == bytes([0] * 256)  # (dense ranks: every tag "other")


def test_registry_stands_in_for_the_subclass():
    # StablePriorityDispatcherSpec.scala:35-40: small integers first, the rest equal, Result last
    spec = lambda t: t if t <= 100 else (101 if t <= 200 else 2 ** 31 - 1)
    Mailboxes.register("com.example.MyPriorityMailbox", lambda c: BoundedStablePriorityMailbox(
        spec, c.get_int("mailbox-capacity"), c.get_duration_s("mailbox-push-timeout-time")))
    try:
        mbs = Mailboxes(CONF)
        m = mbs.lookup("my-prio")
        assert isinstance(m, BoundedStablePriorityMailbox) and m.capacity == 1000
        t = m.priority_table
        assert len(t) == 256 and list(t[:102]) == list(range(102)) and set(t[101:201]) == {101} and t[255] == 102
        with pytest.raises(ConfigurationException, match="push"):
            mbs.lookup("my-prio-blocking")
        with pytest.raises(ConfigurationException, match="NotRegistered"):
            mbs.lookup("unknown-prio")
        with pytest.raises(ConfigurationException, match="built-in"):
            Mailboxes.register("akka.dispatch.BoundedMailbox", lambda c: None)
    finally:
        Mailboxes._registry.pop("com.example.MyPriorityMailbox", None)


def test_priority_tables():
    # dense ranks keep the comparator's order and ties; any Int range fits
    assert priority_table({1: -5, 2: 2 ** 31 - 1, 3: -5})[:4] == bytes([2, 0, 1, 0])  # (tag 0: not given -> last)
    assert priority_table(range(256)) == bytes(range(256))
    assert priority_table(lambda t: 7) == bytes(256)
    with pytest.raises(ConfigurationException):
        priority_table([1, 2, 3])
    with pytest.raises(ConfigurationException):
        priority_table({256: 1})
    u, b = UnboundedPriorityMailbox({5: 0}), BoundedPriorityMailbox({5: 0}, 8, 0)
    assert u.capacity == 0 and b.capacity == 8 and u.priority_table == b.priority_table
    assert u.priority_table[5] == 0 and u.priority_table[6] == 1
    assert isinstance(UnboundedStablePriorityMailbox({}), UnboundedStablePriorityMailbox)
    with pytest.raises(ConfigurationException, match="push"):
        BoundedPriorityMailbox({5: 0}, 8, 10.0)
    with pytest.raises(ConfigurationException):
        UnboundedControlAwareMailbox([300])
