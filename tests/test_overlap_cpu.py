"""CPU: the rule by which the GPU concurrency tests decide that two C calls overlapped (tests/overlap.py), on hand-made intervals."""
import overlap


def test_serialised_calls_give_none():
    assert overlap.pairs([("a", 0, 100), ("b", 150, 250), ("a", 300, 400), ("c", 401, 500)]) == []


def test_touching_ends_give_none():
    assert overlap.pairs([("a", 0, 100), ("b", 100, 200)]) == []
    assert overlap.pairs([("b", 100, 200), ("a", 0, 100)]) == []
    assert overlap.pairs([("a", 0, 100), ("b", 100, 100)]) == []  # (a call of no length overlaps nothing)


def test_a_nested_call_gives_one():
    outer, inner = ("a", 0, 1000), ("b", 400, 500)
    assert overlap.pairs([outer, inner]) == [(outer, inner)]
    assert overlap.pairs([inner, outer]) == [(outer, inner)]  # the order of the input does not matter


def test_the_same_thread_never_pairs_with_itself():
    assert overlap.pairs([("a", 0, 1000), ("a", 400, 500), ("a", 0, 1000)]) == []
    x, y, z = ("a", 0, 1000), ("a", 100, 900), ("b", 200, 800)
    assert sorted(overlap.pairs([x, y, z])) == [(x, z), (y, z)]


def test_half_of_the_shorter_call_is_the_threshold():
    long_call = ("a", 0, 1000)
    assert overlap.pairs([long_call, ("b", 951, 1051)]) == []                               # 49 of 100
    assert overlap.pairs([long_call, ("b", 950, 1050)]) == [(long_call, ("b", 950, 1050))]  # 50 of 100
    # the SHORTER call decides, whichever of the two starts first
    assert overlap.pairs([("b", 0, 100), ("a", 51, 2000)]) == []
    assert overlap.pairs([("b", 0, 100), ("a", 50, 2000)]) == [(("b", 0, 100), ("a", 50, 2000))]
    # an odd length: 2 * common >= shorter, no rounding in the call's favour
    assert overlap.pairs([("a", 0, 101), ("b", 51, 1000)]) == []
    assert overlap.pairs([("a", 0, 101), ("b", 50, 1000)]) != []


def test_many_threads_count_every_pair_once():
    iv = [(t, 0, 100) for t in range(5)]
    assert len(overlap.pairs(iv)) == 10
