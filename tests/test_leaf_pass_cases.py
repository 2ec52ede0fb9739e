"""The cases of tests/leaf_pass_cases.py drive the leaf pass (csrc/rrt_leaf_body.h) past the constants its branches turn on --
asserted with the CPU checker alone, so that it is checked where there is no GPU.  The conditions are fixed by constants in
the kernel's text (64 chain nodes per descriptor chunk, RS_CAP = 256 elements per re-summation window, 2 048 slots in the owner
table), not by measurements."""
import numpy as np
import pytest

import leaf_pass_cases as lp


@pytest.fixture(scope="module")
def shapes(orc):
    """structure() of episode 0 of every case (the checker runs once per case)"""
    out = {n: lp.structure(lp.reference(n), lp.horizon(n)) for n in lp.CASES}
    print("\ncase           leaves  best chain/elements  max chain/elements  slots pruned/swept  depth pruned/swept")
    for n in lp.CASES:
        print(lp.table_row(n))
    return out


def _max(a):
    return int(a.max()) if len(a) else 0


def test_every_case_has_a_best_leaf(shapes):
    for n in lp.CASES:
        r = lp.reference(n)
        assert r["status"] == 0 and r["best_leaf"] >= 1 and r["n_leaves"] == len(shapes[n]["leaves"]) > 0, n
        assert r["best_leaf"] in shapes[n]["leaves"], n
        assert len(r["path"]) == shapes[n]["best_elems"], n  # the course holds one row per element
        assert np.array_equal(r["leaf_cost"][:, 4], shapes[n]["elems"]), n


def test_structure_on_a_hand_made_tree():
    """0 - 1 - 2 - 4 and 0 - 3; node 4 qualifies (horizon 100): chain 4, elements 1 + (1+2) + (1+0) + (1+5); one pass of five
    ids swept, of four pruned (3 is no ancestor); in-pass depth 3"""
    nodes = np.zeros((5, 6))
    nodes[:, 3] = [0.0, 10.0, 20.0, 15.0, 71.0]
    r = dict(nodes=nodes, parent=np.array([-1, 0, 1, 0, 2], np.int32), pt_cnt=np.array([9, 2, 0, 7, 5], np.int32), best_leaf=4)
    s = lp.structure(r, 100.0)
    assert s["leaves"].tolist() == [4] and s["chain"].tolist() == [4] and s["elems"].tolist() == [11]
    assert s["marked"].tolist() == [0, 1, 2, 4]
    assert s["pruned"]["slots"].tolist() == [16] and s["swept"]["slots"].tolist() == [23]
    assert s["pruned"]["depth"].tolist() == [3] and s["swept"]["depth"].tolist() == [3]
    assert (s["best_chain"], s["best_elems"], s["max_chain"], s["max_elems"]) == (4, 11, 4, 11)
    none = lp.structure(dict(r, best_leaf=-1), 500.0)
    assert len(none["leaves"]) == 0 and len(none["marked"]) == 0 and none["best_chain"] == 0
    assert lp.strict_prefix_minima([3.0, 3.0, 2.0, np.nan, 5.0, -np.inf, -np.inf]) == 3


def test_deep(shapes):
    """the second descriptor chunk: a best leaf of >= 65 chain nodes in at least two cases, a qualifying leaf of >= 129 (a
    third chunk) in at least one, and a deep case in time-bin mode (the lim and grid kernels take no other)"""
    deep_best = [n for n in lp.DEEP if shapes[n]["best_chain"] >= lp.CHAIN_CHUNK + 1]
    assert len(deep_best) >= 2, deep_best
    assert any(shapes[n]["max_chain"] >= 2 * lp.CHAIN_CHUNK + 1 for n in lp.DEEP)
    for n in lp.DEEP_TIMEBIN:
        assert lp.CASES[n]["mode"] == "timebin" and shapes[n]["best_chain"] >= lp.CHAIN_CHUNK + 1, n
    for n in lp.DEEP:  # every deep case re-sums some leaf through a second chunk once every leaf is re-summed (the leaf log)
        assert shapes[n]["max_chain"] >= lp.CHAIN_CHUNK + 1, n


def test_long(shapes):
    """the second re-summation window: a best leaf of >= 257 elements; a third: some leaf of >= 513"""
    assert any(shapes[n]["best_elems"] >= lp.RS_CAP + 1 for n in lp.CASES)
    assert any(shapes[n]["max_elems"] >= 2 * lp.RS_CAP + 1 for n in lp.CASES)
    # a window that ends inside a chunk and a chunk that ends inside a window: elements per chunk of 64 nodes on both sides
    s, r = shapes["plan_long"], lp.reference("plan_long")
    per_node = 1 + r["pt_cnt"].astype(np.int64)
    m, chunk = int(r["best_leaf"]), []
    while m >= 0 and len(chunk) < lp.CHAIN_CHUNK:
        chunk.append(per_node[m] if r["parent"][m] >= 0 else 1)
        m = int(r["parent"][m])
    assert sum(chunk) > lp.RS_CAP and s["best_elems"] - sum(chunk) < lp.RS_CAP  # first chunk: two windows; second: one


def test_wide(shapes):
    """the owner search: a pass of > 2 048 point slots under pruning, one with every node swept, one of them > 4 096 (two
    doublings past the table)"""
    assert any(_max(shapes[n]["pruned"]["slots"]) > lp.OWNER_TABLE for n in lp.WIDE)
    assert any(_max(shapes[n]["swept"]["slots"]) > lp.OWNER_TABLE for n in lp.WIDE)
    assert any(max(_max(shapes[n]["pruned"]["slots"]), _max(shapes[n]["swept"]["slots"])) > 2 * lp.OWNER_TABLE for n in lp.WIDE)
    for n in lp.WIDE:
        for route in ("pruned", "swept"):
            assert (shapes[n][route]["slots"] > lp.OWNER_TABLE).any(), (n, route)
    # passes on the near side in the same tree: both owner rules in one episode
    assert any((shapes[n]["pruned"]["slots"] <= lp.OWNER_TABLE).any() for n in lp.WIDE)
    # nodes without points inside a wide pass: they share their successor's first slot, the search must skip them
    r = lp.reference("wide_a")
    ids = shapes["wide_a"]["marked"]
    wide = [ids[i:i + lp.PASS] for i in range(0, len(ids), lp.PASS) if r["pt_cnt"][ids[i:i + lp.PASS]].sum() > lp.OWNER_TABLE]
    assert any((r["pt_cnt"][p][1:] == 0).any() for p in wide) or any((r["pt_cnt"][p] == 0).any() for p in wide)


def test_serial(shapes):
    """the in-pass loops: a pass whose nodes hang on each other 48 deep or more, pruned and swept"""
    assert any(_max(shapes[n]["pruned"]["depth"]) >= 48 for n in lp.CASES)
    # (the marking sweep walks blocks of 64 consecutive ids: its rounds are bounded by the swept depth; past the control's 16)
    assert any(_max(shapes[n]["swept"]["depth"]) >= 16 for n in lp.CASES)
    assert max(_max(shapes[n]["pruned"]["depth"]) for n in lp.CASES) == lp.PASS - 1  # a whole pass in series


def test_control_is_on_the_near_side(shapes):
    """the default-parameter case of tests/test_gpu_rows_kernel.py (o64_default), all of its eight checked episodes: the new
    cases add something"""
    import test_gpu_rows_kernel as rk
    c = rk.CASES["o64_default"]
    assert c["world"] == lp.CASES["control"]["world"] and c["n_iter"] == lp.CASES["control"]["n_iter"] and c["kw"] == {}
    s = shapes["control"]
    assert 0 < s["best_chain"] < lp.CHAIN_CHUNK and s["max_chain"] < lp.CHAIN_CHUNK
    assert 0 < s["best_elems"] < lp.RS_CAP and s["max_elems"] < lp.RS_CAP
    assert _max(s["pruned"]["slots"]) < lp.OWNER_TABLE and _max(s["swept"]["slots"]) < lp.OWNER_TABLE
    assert _max(s["pruned"]["depth"]) < 16 and _max(s["swept"]["depth"]) < 16


def test_leaf_elements_in_the_reference_order_reproduce_the_log(orc):
    """leaf_elements() is the reference's element list: orc.cost over it, all bins selected, reproduces the checker's
    leaf_cost row of the best leaf and of the longest leaf, bit for bit"""
    for n in ("control", "plan_long", "bin_deep_a"):
        r, c = lp.reference(n), lp.CASES[n]
        w = lp.world(n)
        wa = lp.world_arrays(orc, w)
        s = lp.structure(r, lp.horizon(n))
        for k in {int(np.flatnonzero(s["leaves"] == r["best_leaf"])[0]), int(s["elems"].argmax())}:
            leaf = int(s["leaves"][k])
            el = lp.leaf_elements(r, leaf)
            assert len(el) == s["elems"][k]
            got = orc.cost(wa, 0, len(w["bins"]), el, r["nodes"][leaf, 3], c["kw"].get("weights", (-3, -3, -4)), kind="portable")
            assert got.tobytes() == r["leaf_cost"][k, :4].tobytes(), (n, k, got, r["leaf_cost"][k])
