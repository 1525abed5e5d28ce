"""CPU: the recorded-list policy (gfv/listcache.py) driven with fake entries of given `bytes` - no device, no list.  It is held to
the rule as `PoolTrainStep` stated it before the policy had a module of its own: `warm` eager visits of a key, then record, then
replay; least recently used out by bytes while more than one list remains; a key evicted `evict_max` times, or whose list alone
exceeds the budget, stays eager for good; an invalidated key warms up again from its first eager step; `clear` never forgets what
the byte budget has decided."""
import pytest

from gfv.listcache import EVICT_MAX, WARM, Entry, ListCache


def _visit(c, key, nbytes=10, listed=True):
    """One step of `key` as a user of the cache takes it -> the decision."""
    what = c.decide(key, listed)
    if what == "record":
        c.store(key, Entry(object(), nbytes))
    return what


def _stats(c, replayed, recorded, eager, lists, list_bytes):
    assert c.stats() == dict(replayed=replayed, recorded=recorded, eager=eager, lists=lists, list_bytes=list_bytes), c.stats()


def test_constants_and_the_classes_that_name_them():
    from gfv.evaluate import Evaluate
    from gfv.pool_trainer import PoolTrainStep
    from gfv.rollout import Rollout
    from gfv.sweep import Sweep
    assert (WARM, EVICT_MAX) == (2, 2)
    assert Rollout.WARM == Sweep.WARM == Evaluate.WARM == PoolTrainStep.WARM == WARM
    assert Sweep.EVICT_MAX == Evaluate.EVICT_MAX == PoolTrainStep.EVICT_MAX == EVICT_MAX


def test_one_key_warms_up_twice_records_once_and_replays_forever():
    c = ListCache(100)
    assert [_visit(c, "a") for _ in range(7)] == ["eager", "eager", "record"] + ["replay"] * 4
    _stats(c, replayed=4, recorded=1, eager=2, lists=1, list_bytes=10)
    c = ListCache(100, warm=3)
    assert [_visit(c, "a") for _ in range(5)] == ["eager"] * 3 + ["record", "replay"]


def test_not_listed_is_always_eager_and_counts_no_warm_up():
    c = ListCache(100)
    assert [_visit(c, "a", listed=False) for _ in range(5)] == ["eager"] * 5
    assert c.warm == {} and len(c) == 0
    _stats(c, replayed=0, recorded=0, eager=5, lists=0, list_bytes=0)
    assert [_visit(c, "a") for _ in range(4)] == ["eager", "eager", "record", "replay"]      # (the warm-up starts only now)
    assert _visit(c, "a", listed=False) == "eager" and "a" in c                              # (... and the list stays)
    assert _visit(c, "a") == "replay"


@pytest.mark.parametrize("budget", [0, -1])
def test_a_budget_of_nothing_lists_nothing(budget):
    c = ListCache(budget)
    assert [_visit(c, "a") for _ in range(5)] == ["eager"] * 5
    assert c.warm == {} and c.oversize == set()
    _stats(c, replayed=0, recorded=0, eager=5, lists=0, list_bytes=0)


def _warmed(c, keys, nbytes=10):
    for k in keys:
        assert [_visit(c, k, nbytes) for _ in range(WARM)] == ["eager"] * WARM


def test_budget_of_two_lists_three_keys_least_recently_used_goes_out():
    c = ListCache(20)
    _warmed(c, "abc")
    assert [_visit(c, k) for k in "ab"] == ["record", "record"] and list(c) == ["a", "b"]
    assert _visit(c, "a") == "replay" and list(c) == ["b", "a"]          # a replay refreshes recency
    assert _visit(c, "c") == "record" and list(c) == ["a", "c"]          # ... so b, not a, goes out
    assert c.evicted == {"b": 1} and c.oversize == set()
    _stats(c, replayed=1, recorded=3, eager=6, lists=2, list_bytes=20)
    # b is warm: it records at once, and a (least recently used) goes out; then a, and c goes out; ...
    assert _visit(c, "b") == "record" and list(c) == ["c", "b"] and c.evicted == {"b": 1, "a": 1}
    assert _visit(c, "a") == "record" and list(c) == ["b", "a"] and c.evicted == {"b": 1, "a": 1, "c": 1}
    assert _visit(c, "c") == "record" and list(c) == ["a", "c"] and c.evicted == {"b": 2, "a": 1, "c": 1}
    # b has lost its list EVICT_MAX times: eager from now on, and the lists of the others are left alone
    assert c.oversize == {"b"}
    assert [_visit(c, "b") for _ in range(4)] == ["eager"] * 4 and list(c) == ["a", "c"]
    assert [_visit(c, k) for k in "ac"] == ["replay", "replay"]
    _stats(c, replayed=3, recorded=6, eager=10, lists=2, list_bytes=20)


def test_two_keys_alternating_on_a_budget_of_one_do_not_record_on_every_visit():
    c = ListCache(15)
    seen = [_visit(c, k) for k in "ab" * 10]
    assert c.stats()["recorded"] <= 5 and c.stats()["lists"] == 1 and c.stats()["list_bytes"] <= 15, (seen, c.stats())
    assert len(c.oversize) == 1 and set(seen[-6:]) == {"eager", "replay"}


def test_an_entry_larger_than_the_budget_is_not_kept_and_its_key_stays_eager():
    c = ListCache(25)
    _warmed(c, "ab")
    assert _visit(c, "a") == "record"
    kept = c["a"]
    assert c.decide("b") == "record" and c.store("b", Entry(object(), 26)) is False
    assert c.oversize == {"b"} and list(c) == ["a"] and c["a"] is kept and c.evicted == {}
    assert [_visit(c, "b", 1) for _ in range(4)] == ["eager"] * 4          # for good, whatever it would need now
    assert _visit(c, "a") == "replay"
    _stats(c, replayed=1, recorded=2, eager=8, lists=1, list_bytes=10)
    assert c.store("c", Entry(object(), 25)) is True                        # (exactly the budget fits; a goes out for it)
    assert list(c) == ["c"] and c.evicted == {"a": 1}


def test_the_last_list_is_never_evicted():
    c = ListCache(10)
    _warmed(c, "ab")
    assert _visit(c, "a") == "record" and list(c) == ["a"]
    assert _visit(c, "b") == "record" and list(c) == ["b"] and c.evicted == {"a": 1}       # the newest one is the one that stays
    assert _visit(c, "b") == "replay"
    _stats(c, replayed=1, recorded=2, eager=4, lists=1, list_bytes=10)


def test_invalidate_then_one_eager_step_then_record():
    """As `PoolTrainStep.step` made it: the list is dropped and the warm count set to 0 BEFORE the decision, so the step that found
    the stale list is warm-up 1, the next one warm-up 2, and the third visit records."""
    c = ListCache(100)
    assert [_visit(c, "a") for _ in range(4)] == ["eager", "eager", "record", "replay"]
    c.invalidate("a")
    assert "a" not in c and c.warm["a"] == 0
    assert [_visit(c, "a") for _ in range(4)] == ["eager", "eager", "record", "replay"]
    _stats(c, replayed=2, recorded=2, eager=4, lists=1, list_bytes=10)
    assert c.evicted == {} and c.oversize == set()                           # (an invalidation is no eviction)
    with pytest.raises(KeyError):
        c.invalidate("b")


def test_clear_keeps_or_resets_the_warm_counts_and_never_the_byte_decisions():
    c = ListCache(20)
    _warmed(c, "ab")
    assert [_visit(c, k) for k in "ab"] == ["record", "record"]
    c.oversize.add("z")
    c.evicted["y"] = 1
    c.clear(keep_warm=True)
    assert len(c) == 0 and not c and c.warm == {"a": 2, "b": 2}
    assert _visit(c, "a") == "record"                                        # a warmed key records on its next visit
    c.clear(keep_warm=False)
    assert len(c) == 0 and c.warm == {}
    assert [_visit(c, "a") for _ in range(3)] == ["eager", "eager", "record"]
    c.clear()                                                                # (the default: as keep_warm=False)
    assert c.warm == {} and c.oversize == {"z"} and c.evicted == {"y": 1}
    assert [_visit(c, "z") for _ in range(3)] == ["eager"] * 3
    _stats(c, replayed=0, recorded=4, eager=9, lists=0, list_bytes=0)


def test_clear_resets_the_very_dictionary_its_owner_may_hold():
    c = ListCache(20)
    warm = c.warm
    _warmed(c, "a")
    c.clear()
    assert c.warm is warm and warm == {}


def test_unbounded_never_evicts_and_never_marks_a_key_oversize():
    c = ListCache(None)
    for k in range(20):
        assert [_visit(c, k, 1 << 40) for _ in range(4)] == ["eager", "eager", "record", "replay"]
    assert len(c) == 20 and c.oversize == set() and c.evicted == {}
    _stats(c, replayed=20, recorded=20, eager=40, lists=20, list_bytes=20 << 40)


def test_unbounded_over_the_two_keys_of_a_train_step():
    """`TrainStep._lists` is `ListCache(None)` over (accumulate, distributed): the Normalizer's accumulating steps under one key, the
    steady ones under the other.  The script is a `TrainStep(use_graph="list")` on a model that accumulates three times, whose engine
    signature then moves twice (the owner's `invalidate` in front of the decision) and whose guard is switched on at the end
    (`_drop_recorded`: `clear`)."""
    ACC, STEADY = (True, False), (False, False)
    c = ListCache(None)
    assert [_visit(c, ACC, 1 << 40) for _ in range(3)] == ["eager", "eager", "record"] and list(c) == [ACC]
    assert [_visit(c, STEADY, 1 << 40) for _ in range(4)] == ["eager", "eager", "record", "replay"]
    assert list(c) == [ACC, STEADY] and c.warm == {ACC: 2, STEADY: 2}        # (no budget: the older list stays)
    _stats(c, replayed=1, recorded=2, eager=4, lists=2, list_bytes=2 << 40)
    c.invalidate(STEADY)                                                       # the step that finds the list stale ...
    assert list(c) == [ACC] and c.warm == {ACC: 2, STEADY: 0}
    assert _visit(c, STEADY) == "eager" and c.warm[STEADY] == 1                # ... is the first of the new warm-up
    assert STEADY not in c and [_visit(c, STEADY) for _ in range(3)] == ["eager", "record", "replay"]
    c.invalidate(STEADY)
    assert _visit(c, STEADY, listed=False) == "eager" and c.warm[STEADY] == 0  # (a step that is not listed warms nothing up)
    assert [_visit(c, STEADY) for _ in range(3)] == ["eager", "eager", "record"]
    assert c[ACC].bytes == 1 << 40 and c.oversize == set() and c.evicted == {}  # the other key's list was never touched
    _stats(c, replayed=2, recorded=4, eager=9, lists=2, list_bytes=(1 << 40) + 10)
    c.clear()
    assert not c and c.warm == {}
    assert [_visit(c, STEADY) for _ in range(4)] == ["eager", "eager", "record", "replay"]
    _stats(c, replayed=3, recorded=5, eager=11, lists=1, list_bytes=10)


def test_the_mapping_view():
    c = ListCache(100)
    assert not c and len(c) == 0 and "a" not in c and list(c) == []
    _warmed(c, "abc")
    ents = {}
    for k in "abc":
        assert c.decide(k) == "record"
        ents[k] = Entry(object(), 10, outs=(k,), early=k.upper())
        assert c.store(k, ents[k]) is True
    assert c and len(c) == 3 and "a" in c and "z" not in c
    assert c.decide("a") == "replay"
    assert list(c) == ["b", "c", "a"] == list(c.keys())                      # iteration order = recency, oldest first
    assert list(c.values()) == [ents["b"], ents["c"], ents["a"]]
    assert list(c.items()) == [(k, ents[k]) for k in "bca"]
    assert c["a"] is ents["a"] and c.get("z") is None and dict(c) == ents
    assert sorted(e.bytes for e in c.values()) == [10, 10, 10]
    assert (c["a"].outs, c["a"].early, c["a"].bytes) == (("a",), "A", 10)   # the caller's own fields beside cl / bytes / outs
