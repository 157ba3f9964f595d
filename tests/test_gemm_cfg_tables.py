"""The conv GEMM cfg tables (csrc/kernels/gemm_cfg.h), read back through the host-only op
hcb.gemm_cfg_table of both kernel builds, against the Python planner's literal tables
(ops/functional.py), the cfgs the inference tests sweep, and a pinned copy of every row."""
import os

import pytest

from azure_hc_intel_tf_amd.ops import autotune
from azure_hc_intel_tf_amd.ops import functional as Fn

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "azure_hc_intel_tf_amd")
BUILDS = [("_hcb_kernels.so", "hcb"), ("_hcb_kernels_f16.so", "hcb16")]
COLS = ("cfg", "kind", "wm", "wn", "tm", "tn", "kw", "nst", "occ", "extra", "fb", "inf")
# launcher kinds (gemm_cfg.h GemmKind; 6 was the stream-K kernels' and stays unused)
REG, GLDS, PATCH, KQ, TILE, PERSIST = range(6)
BRES, RETIRED = 7, 8

# Every row of every family, (kind, WM, WN, TM, TN, slot depth, ring slots, occupancy, PMAX / KS, fallback),
# as the launch switches of the commit before the tables spelled them. A cfg number stored in
# tuned/*.json means its row: a change to this literal (a row added, removed, renumbered or given other
# template arguments) needs a new autotune.CACHE_VERSION, and the version below changed with it.
PINNED_CACHE_VERSION = 6
PINNED = {
    "conv": {
        0: (REG, 2, 2, 64, 64, 64, 0, 1, 0, -1), 1: (REG, 4, 1, 32, 64, 64, 0, 1, 0, -1),
        2: (REG, 2, 2, 32, 32, 64, 0, 1, 0, -1), 3: (REG, 1, 4, 64, 32, 64, 0, 1, 0, -1),
        4: (GLDS, 2, 2, 64, 64, 64, 3, 1, 0, -1), 5: (GLDS, 4, 1, 32, 64, 64, 3, 1, 0, -1),
        6: (GLDS, 2, 2, 32, 32, 64, 4, 1, 0, -1), 7: (GLDS, 1, 4, 64, 32, 64, 3, 1, 0, -1),
        8: (GLDS, 2, 2, 64, 64, 64, 4, 1, 0, -1), 9: (GLDS, 2, 2, 64, 64, 64, 5, 1, 0, -1),
        10: (GLDS, 4, 1, 32, 64, 64, 6, 1, 0, -1), 11: (GLDS, 1, 4, 64, 32, 64, 6, 1, 0, -1),
        12: (GLDS, 2, 4, 64, 32, 64, 3, 1, 0, -1), 13: (GLDS, 4, 2, 32, 64, 64, 3, 1, 0, -1),
        14: (GLDS, 4, 2, 64, 64, 64, 3, 1, 0, -1), 15: (GLDS, 2, 4, 64, 64, 64, 3, 1, 0, -1),
        16: (GLDS, 2, 4, 32, 32, 64, 4, 1, 0, -1),
        17: (PATCH, 2, 4, 64, 32, 64, 3, 1, 8, 13), 18: (PATCH, 4, 2, 64, 64, 64, 3, 1, 8, 14),
        19: (PATCH, 4, 2, 64, 32, 64, 3, 1, 8, 14), 20: (PATCH, 2, 2, 64, 32, 64, 3, 1, 16, 5),
        21: (PATCH, 2, 4, 64, 32, 64, 4, 1, 8, 13),
    },
    "wgrad": {
        0: (REG, 2, 2, 64, 64, 64, 0, 1, 0, -1), 1: (REG, 1, 4, 64, 32, 64, 0, 1, 0, -1),
        2: (REG, 2, 2, 32, 32, 64, 0, 1, 0, -1),
        3: (GLDS, 2, 2, 64, 64, 64, 4, 1, 0, -1), 4: (GLDS, 2, 4, 64, 32, 64, 3, 1, 0, -1),
        5: (GLDS, 4, 2, 64, 64, 64, 3, 1, 0, -1), 6: (GLDS, 2, 4, 64, 64, 64, 3, 1, 0, -1),
        7: (GLDS, 2, 4, 32, 32, 64, 4, 1, 0, -1), 8: (GLDS, 2, 2, 32, 32, 64, 4, 1, 0, -1),
        9: (GLDS, 1, 4, 64, 32, 64, 4, 1, 0, -1),
        10: (KQ, 1, 1, 64, 64, 64, 0, 1, 4, -1), 11: (KQ, 2, 1, 64, 64, 64, 0, 1, 2, -1),
        12: (KQ, 1, 2, 64, 64, 64, 0, 1, 2, -1),
        13: (REG, 2, 2, 64, 32, 64, 0, 1, 0, -1), 14: (REG, 2, 2, 32, 64, 64, 0, 1, 0, -1),
    },
    "p3": {
        0: (TILE, 2, 2, 64, 32, 64, 2, 1, 0, -1), 1: (TILE, 2, 2, 32, 64, 64, 2, 1, 0, -1),
        2: (TILE, 4, 2, 32, 32, 64, 2, 1, 0, -1), 3: (TILE, 2, 4, 32, 32, 64, 2, 1, 0, -1),
        4: (TILE, 2, 2, 32, 32, 64, 2, 1, 0, -1), 5: (TILE, 4, 1, 32, 64, 64, 2, 1, 0, -1),
        6: (TILE, 1, 4, 64, 32, 64, 2, 1, 0, -1), 7: (TILE, 2, 4, 64, 32, 32, 3, 1, 0, -1),
        8: (TILE, 4, 2, 32, 64, 32, 3, 1, 0, -1), 9: (TILE, 2, 2, 64, 64, 32, 3, 1, 0, -1),
        10: (TILE, 4, 2, 64, 64, 32, 2, 1, 0, -1), 11: (TILE, 2, 4, 64, 64, 32, 2, 1, 0, -1),
        12: (TILE, 2, 2, 32, 64, 32, 4, 1, 0, -1), 13: (TILE, 2, 2, 64, 32, 32, 4, 1, 0, -1),
        14: (TILE, 2, 2, 64, 32, 32, 2, 2, 0, -1), 15: (TILE, 2, 2, 32, 64, 32, 2, 2, 0, -1),
        16: (TILE, 2, 2, 32, 32, 32, 3, 2, 0, -1), 17: (TILE, 2, 2, 32, 32, 32, 2, 3, 0, -1),
        18: (PERSIST, 2, 2, 32, 64, 32, 2, 2, 0, 15), 19: (PERSIST, 2, 2, 64, 32, 32, 2, 2, 0, 14),
        20: (PERSIST, 2, 2, 32, 32, 32, 3, 2, 0, 16), 21: (PERSIST, 2, 2, 32, 32, 32, 2, 3, 0, 17),
        22: (PERSIST, 2, 4, 64, 32, 32, 3, 1, 0, 7),
        # retired (the stream-K numbers): no kernel of their own; the geometry of the cfgs they run
        23: (RETIRED, 2, 2, 32, 64, 32, 2, 2, 0, 18), 24: (RETIRED, 2, 2, 64, 32, 32, 2, 2, 0, 19),
        25: (RETIRED, 2, 2, 32, 32, 32, 3, 2, 0, 20), 26: (RETIRED, 2, 2, 32, 32, 32, 2, 3, 0, 21),
        27: (RETIRED, 2, 4, 64, 32, 32, 3, 1, 0, 22), 28: (RETIRED, 4, 2, 32, 64, 32, 3, 1, 0, 8),
        29: (RETIRED, 4, 2, 64, 64, 32, 2, 1, 0, 10), 30: (RETIRED, 2, 4, 64, 64, 32, 2, 1, 0, 11),
        31: (BRES, 1, 4, 64, 64, 32, 3, 1, 0, 18), 32: (BRES, 2, 4, 64, 64, 32, 2, 1, 0, 18),
        33: (BRES, 2, 2, 32, 32, 32, 3, 1, 0, 20), 34: (BRES, 2, 2, 64, 32, 32, 2, 1, 0, 19),
        35: (BRES, 4, 2, 32, 32, 32, 2, 1, 0, 19), 36: (BRES, 4, 2, 32, 64, 32, 2, 1, 0, 22),
    },
    "wgrad_p3": {
        0: (TILE, 2, 2, 64, 32, 64, 2, 1, 0, -1), 1: (TILE, 2, 2, 32, 64, 64, 2, 1, 0, -1),
        2: (TILE, 2, 2, 32, 32, 64, 3, 1, 0, -1), 3: (TILE, 4, 2, 32, 32, 64, 2, 1, 0, -1),
        4: (TILE, 2, 4, 32, 32, 64, 2, 1, 0, -1), 5: (TILE, 2, 2, 32, 32, 64, 2, 1, 0, -1),
        6: (TILE, 2, 4, 64, 32, 32, 3, 1, 0, -1), 7: (TILE, 4, 2, 32, 64, 32, 3, 1, 0, -1),
        8: (TILE, 4, 2, 64, 64, 32, 2, 1, 0, -1), 9: (TILE, 2, 4, 64, 64, 32, 2, 1, 0, -1),
        10: (TILE, 2, 2, 64, 64, 32, 3, 1, 0, -1), 11: (TILE, 2, 2, 64, 32, 32, 3, 1, 0, -1),
        12: (TILE, 2, 2, 64, 32, 32, 2, 2, 0, -1), 13: (TILE, 2, 2, 32, 64, 32, 2, 2, 0, -1),
        14: (TILE, 2, 2, 32, 32, 32, 3, 2, 0, -1), 15: (TILE, 2, 2, 32, 32, 32, 2, 3, 0, -1),
        16: (PERSIST, 2, 2, 64, 32, 32, 2, 2, 0, -1), 17: (PERSIST, 2, 2, 32, 64, 32, 2, 2, 0, -1),
        18: (PERSIST, 2, 2, 32, 32, 32, 2, 3, 0, -1),
    },
}


@pytest.fixture(scope="module", params=BUILDS, ids=[ns for _, ns in BUILDS])
def tables(request):
    """family -> {cfg: row dict} of one kernel build."""
    import torch

    name, ns = request.param
    path = os.path.join(PKG, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not built (python __graft_entry__.py builds it)")
    torch.ops.load_library(path)
    op = getattr(torch.ops, ns).gemm_cfg_table
    out = {}
    for fam in PINNED:
        flat = list(op(fam))
        assert len(flat) % len(COLS) == 0
        rows = [dict(zip(COLS, flat[i:i + len(COLS)])) for i in range(0, len(flat), len(COLS))]
        assert [r["cfg"] for r in rows] == list(range(len(rows)))
        out[fam] = {r["cfg"]: r for r in rows}
    return out


def _tiles(rows):
    return {c: (r["wm"] * r["tm"], r["wn"] * r["tn"]) for c, r in rows.items()}


def test_python_tile_tables_equal_the_exported_tiles(tables):
    assert Fn._CONV_TILES == _tiles(tables["conv"])
    assert Fn._WGRAD_TILES == _tiles(tables["wgrad"])
    assert Fn._WP3_TILES == _tiles(tables["wgrad_p3"])
    p3 = _tiles(tables["p3"])
    retired = {c for c, r in tables["p3"].items() if r["kind"] == RETIRED}
    assert retired == set(range(23, 31)) and not retired & set(Fn._P3_TILES)
    assert Fn._P3_TILES == {c: t for c, t in p3.items() if c not in retired}
    assert Fn.PATCH_CFGS == tuple(c for c, r in tables["conv"].items() if r["kind"] == PATCH)
    assert Fn.PATCH_CFG0 == min(Fn.PATCH_CFGS)


def test_occupancy_and_resident_ring_slots(tables):
    # (a retired row keeps the columns of the kernel it had; the planner lists launchable cfgs only)
    assert Fn._P3_OCC == {c: r["occ"] for c, r in tables["p3"].items() if r["occ"] != 1 and r["kind"] != RETIRED}
    assert Fn._WP3_OCC == {c: r["occ"] for c, r in tables["wgrad_p3"].items() if r["occ"] != 1}
    assert Fn._P3_BRES == {c: r["nst"] for c, r in tables["p3"].items() if r["kind"] == BRES}


def test_fallbacks(tables):
    conv, p3 = tables["conv"], tables["p3"]
    assert Fn._PATCH_TWIN == {c: r["fb"] for c, r in conv.items() if r["kind"] == PATCH}
    assert all((r["fb"] >= 0) == (r["kind"] == PATCH) for r in conv.values())

    def per_tile(c):
        while p3[c]["kind"] != TILE:
            c = p3[c]["fb"]
        return c

    assert all((r["fb"] >= 0) == (r["kind"] != TILE) for r in p3.values())
    assert Fn._P3_PERSIST == {c: per_tile(c) for c, r in p3.items() if r["kind"] not in (TILE, RETIRED)}
    retired = {c: per_tile(c) for c, r in p3.items() if r["kind"] == RETIRED}
    assert retired == {23: 15, 24: 14, 25: 16, 26: 17, 27: 7, 28: 8, 29: 10, 30: 11} == Fn._P3_RETIRED
    # a patch twin keeps the row tile, so a per-tile statistics slab keeps its size
    assert all(r["wm"] * r["tm"] == conv[r["fb"]]["wm"] * conv[r["fb"]]["tm"] for r in conv.values() if r["fb"] >= 0)
    assert all(r["fb"] == -1 for fam in ("wgrad", "wgrad_p3") for r in tables[fam].values())


def test_inference_cfgs_are_the_swept_ones(tables):
    import test_infer_fused_gpu as T

    assert [c for c, r in tables["conv"].items() if r["inf"]] == T.A16_CFGS
    assert [c for c, r in tables["p3"].items() if r["inf"]] == T.P3_CFGS
    assert not any(r["inf"] for fam in ("wgrad", "wgrad_p3") for r in tables[fam].values())


def test_pinned_tables(tables):
    assert autotune.CACHE_VERSION == PINNED_CACHE_VERSION, "a new cache version: re-pin the tables with it"
    for fam, want in PINNED.items():
        got = {c: tuple(r[k] for k in COLS[1:-1]) for c, r in tables[fam].items()}
        assert got == want, f"{fam}: the cfg table changed -- bump autotune.CACHE_VERSION and re-pin"
