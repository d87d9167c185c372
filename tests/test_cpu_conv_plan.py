"""The shapes test_gpu_conv_tiles.py runs really are on the block tiles their rows claim.  conv_cases.py restates conv_tile /
conv_plan / conv_eval_plan; here the restatement is held against sed_conv3x3_plan (the plan the launches read) on a dense sweep,
every row of the enumerated table against that query, and the table as a whole must cover every tile the sweep returns.  No GPU."""
import numpy as np
import pytest

import conv_cases as cc  # noqa: E402

FIELDS = ("kind", "TT", "FT", "nft", "nct", "tblocks", "rows", "xcd_order")


@pytest.fixture(scope="module")
def ops():
    from sed_crnn_amd import ops as o
    return o


@pytest.mark.parametrize("nct", [4, 2, 1])
def test_restated_conv_tile_equals_the_library_on_a_dense_sweep(ops, nct):
    """F 1..256 x T 1..128 under the row limit of each output-channel width, every field of the query"""
    Cout = cc.COUT_OF_NCT[nct]
    TT, FT, NF, _ = cc.tile_sweep(cc.limit_of(nct))
    assert TT[1:, 1:].min() > 0                                    # a 1 x 2 tile always fits: the MFMA path takes every shape
    for F in range(1, cc.SWEEP_F + 1):
        for T in range(1, cc.SWEEP_T + 1):
            p = ops.conv3x3_plan(3, cc.CV_CIC, F, T, Cout)
            tb = cc.cdiv(T, int(TT[F, T]))
            want = dict(kind=1, TT=TT[F, T], FT=FT[F, T], nft=NF[F, T], nct=nct, tblocks=tb, rows=3 * tb * NF[F, T], xcd_order=0)
            assert p == want, (F, T, p, want)


def test_restated_pooled_inference_plan_equals_the_library_on_a_dense_sweep(ops):
    TT, FT, NF = cc.eval_sweep()
    n = 0
    for F in range(1, cc.SWEEP_F + 1):
        for T in range(1, cc.SWEEP_T + 1):
            p = ops.conv3x3_plan(8, cc.CV_CIC, F, T, 128, False, 1)
            if TT[F, T] == 0:
                assert p == dict.fromkeys(FIELDS, 0) | dict(kind=-1), (F, T, p)
            else:
                tb = cc.cdiv(T, int(TT[F, T]))
                assert p == dict(kind=1, TT=TT[F, T], FT=FT[F, T], nft=NF[F, T], nct=4, tblocks=tb, rows=8 * tb * NF[F, T], xcd_order=1), (F, T, p)
                assert TT[F, T] % 2 == 0 and FT[F, T] <= 32
                n += 1
            assert bool(ops.lib().sed_conv3x3_bn_relu_pool_eval_supported(8, cc.CV_CIC, F, T, 128)) == (TT[F, T] > 0)
    assert 0 < n < cc.SWEEP_F * cc.SWEEP_T                          # both answers occur
    # only 128-wide output takes the pooled kernel
    assert ops.conv3x3_plan(2, 32, 40, 16, 64, False, 1)["kind"] == -1 and ops.conv3x3_plan(2, 32, 40, 16, 128, False, 1)["kind"] == 1


def test_scalar_restatement_equals_the_swept_one_and_the_library(ops):
    """conv_plan / conv_eval_plan as plain loops (what a reader checks against conv.hip) on every 7th shape of the sweep, on other
    channel counts and batches, and off the MFMA path"""
    sweeps = {nct: cc.tile_sweep(cc.limit_of(nct)) for nct in (4, 2, 1)}
    eTT, eFT, eNF = cc.eval_sweep()
    k = 0
    for F in range(1, cc.SWEEP_F + 1):
        for T in range(1, cc.SWEEP_T + 1):
            k += 1
            if k % 7:
                continue
            for nct in (4, 2, 1):
                t = cc.conv_tile(F, T, cc.limit_of(nct))
                TT, FT, NF, SC = sweeps[nct]
                assert t == (TT[F, T], FT[F, T], NF[F, T], SC[F, T]), (F, T, nct)
            e = cc.conv_eval_plan(8, 32, F, T, 128)
            assert (e["TT"], e["FT"], e["nft"]) == (eTT[F, T], eFT[F, T], eNF[F, T]), (F, T)
    for B, Cin, F, T, Cout, nchw in [(16, 128, 40, 256, 128, False), (128, 128, 128, 64, 128, False), (8, 64, 40, 16, 256, False), (9, 96, 20, 31, 192, False),
                                     (24, 32, 8, 100, 96, False), (2, 1, 40, 16, 128, True), (8, 16, 40, 10, 16, False), (3, 100, 10, 6, 100, False),
                                     (2, 128, 40, 16, 128, True), (2, 3, 40, 2, 6, False), (2, 32, 7000, 4, 30, False)]:
        for which in ((0, 1) if not nchw else (0,)):
            p = ops.conv3x3_plan(B, Cin, F, T, Cout, nchw, which)
            r = cc.conv_eval_plan(B, Cin, F, T, Cout) if which else cc.conv_plan(B, Cin, F, T, Cout, nchw)
            assert p == {f: r[f] for f in FIELDS}, (B, Cin, F, T, Cout, nchw, which, p)
    # the remap is on exactly when the MFMA kernel sees a batch that is a multiple of 8
    assert [ops.conv3x3_plan(B, 32, 40, 8, 128)["xcd_order"] for B in (1, 7, 8, 9, 16, 24, 128)] == [0, 0, 1, 0, 1, 1, 1]
    assert ops.conv3x3_plan(8, 1, 40, 8, 128, True)["xcd_order"] == 0
    # the row count of the query is the one the launches allocate by
    L = ops.lib()
    assert L.sed_conv3x3_stat_rows(8, 32, 61, 9, 128, 0) == ops.conv3x3_plan(8, 32, 61, 9, 128)["rows"] == 8 * 2 * 2
    assert L.sed_conv3x3_dgrad_bnred_rows(8, 128, 61, 9, 128) == 32


def test_plan_query_rejects_bad_arguments(ops):
    from sed_crnn_amd._lib import SedHipError
    for args in ((0, 32, 8, 8, 32, 0, 0), (1, 0, 8, 8, 32, 0, 0), (1, 32, 0, 8, 32, 0, 0), (1, 32, 8, 0, 32, 0, 0), (1, 32, 8, 8, 0, 0, 0),
                 (1, 32, 8, 8, 32, 0, 2), (1, 32, 8, 8, 32, 0, -1), (1, 32, 8, 8, 128, 1, 1)):
        with pytest.raises(SedHipError):
            ops.conv3x3_plan(*args)
    assert ops.lib().sed_conv3x3_plan(1, 32, 8, 8, 32, 0, 0, None) != 0


ALL_ROWS = cc.build_table()[0]


@pytest.mark.parametrize("name", [r["name"] for r in ALL_ROWS])
def test_row_is_on_the_tile_it_claims(ops, name):
    r = cc.row(name)
    F, T, nct, which = r["F"], r["T"], r["nct"], r["which"]
    Cout = cc.COUT_OF_NCT[nct]
    for B in (cc.B_PLAIN, cc.B_XCD):
        p = ops.conv3x3_plan(B, cc.CV_CIC, F, T, Cout, False, which)
        facts = dict(tile=(p["TT"], p["FT"]), nft=p["nft"], nct=p["nct"], tblocks=p["tblocks"],
                     ragged_f=p["nft"] * p["FT"] > F, ragged_t=T % p["TT"] != 0)
        assert p["kind"] == 1
        for key, got in facts.items():
            assert got == r[key], f"row {name}, B = {B}: {key} is {got}, the row claims {r[key]}"
        assert p["rows"] == B * p["tblocks"] * p["nft"] and p["xcd_order"] == int(B == cc.B_XCD)
        # the size bound that keeps a GPU case far below a second (18 * Cin flop per output element: 0.6 GFLOP at Cin = 32)
        assert B * T * F * Cout <= cc.MAX_OUT_ELEMS
        # the data gradient of the GPU test (a Cin -> 32 conv whose gradient has Cout channels) and the 128-channel plans of
        # the epilogue tests read the same tile: it depends on F, T and the output width alone
        assert ops.conv3x3_plan(B, 128, F, T, Cout, False, which) == p
    if r["kind"] == "interior":                # the epilogue's unchecked path: every tile wholly inside, whole 32-row MFMA tiles
        assert not r["ragged_f"] and not r["ragged_t"] and (r["tile"][0] * r["tile"][1]) % 32 == 0
    if r["kind"] == "grid":
        assert r["nft"] * r["tblocks"] >= 3
    # exactness precondition of the integer tests: |y| <= 9 * Cin * 3 + 3 (x in [-3, 3], w in {-1, 0, 1}, |bias| <= 3)
    assert 9 * cc.CV_CIC * 3 + 3 < 2 ** 24 and 9 * 128 * 3 + 3 < 2 ** 24


def test_the_table_covers_every_tile_the_sweep_returns(ops):
    rows, returned = cc.build_table()
    assert len({r["name"] for r in rows}) == len(rows)
    # the sets the table was enumerated from are the library's own
    for (nct, which), tiles in returned.items():
        got = set()
        for F in range(1, cc.SWEEP_F + 1):
            for T in range(1, cc.SWEEP_T + 1):
                p = ops.conv3x3_plan(3, 32, F, T, cc.COUT_OF_NCT[nct], False, which)
                if p["kind"] == 1:
                    got.add((p["TT"], p["FT"]))
        assert got == tiles, (nct, which)
    base = returned[(4, 0)]
    covered = {r["tile"] for r in cc.rows(4, 0, "tile")}
    print(f"\nlimit 160 (Cout % 128 == 0): the sweep returns {len(base)} distinct tiles, the table covers {len(covered & base)}")
    assert covered == base
    for nct in (2, 1):
        only = returned[(nct, 0)] - base
        have = {r["tile"] for r in cc.rows(nct, 0, "tile")}
        print(f"limit {cc.limit_of(nct)} (nct {nct}): {len(only)} tiles that limit 160 never returns, all covered; + {sorted(have - only)}")
        assert have == only | (set(cc.NAMED_TILES) & returned[(nct, 0)])
        assert set(cc.NAMED_TILES) <= have                          # 5x32, 8x20, 20x8 and 35x4 exist under the wider limits too
        assert all(t[0] * t[1] > 160 for t in only) and max(t[0] * t[1] for t in only) == 196
    pool = {r["tile"] for r in cc.rows(4, 1)}
    print(f"pooled inference plan: the sweep returns {len(returned[(4, 1)])} distinct tiles, the table covers {len(pool)}")
    assert pool == returned[(4, 1)]
    # what the issue found missing is in: the model's F = 128 tile, a halo tile at the staging budget, a one-row tile of 82 columns,
    # tall tiles, tiles above 160 rows, shapes with more than one tile per sequence in both directions, wholly-interior shapes
    assert (5, 32) in base and (1, 82) in base and max(t[1] for t in base if t[0] == 1) == 82
    assert any(cc.halo_edge(t) for t in base) and any(cc.halo_edge(r["tile"]) for r in cc.rows(2)) and any(cc.halo_edge(r["tile"]) for r in cc.rows(1))
    assert len({t for t in base if t[0] > 8}) > 50
    assert any(r["nft"] > 1 and r["tblocks"] > 1 for r in cc.rows(4)) and any(r["nft"] > 1 and r["tblocks"] > 1 for r in cc.rows(1))
    assert len(cc.rows(4, 0, "interior")) >= 20
    assert sum(r["ragged_t"] for r in rows) >= 50 and sum(r["ragged_f"] for r in rows) >= 50


def _coverage():
    rows, returned = cc.build_table()
    out = []
    for (nct, which), tiles in sorted(returned.items()):
        have = {r["tile"] for r in rows if (r["nct"], r["which"]) == (nct, which)}
        want = tiles if (nct == 4) else (tiles - returned[(4, 0)]) | (set(cc.NAMED_TILES) & tiles)
        what = "pooled plan" if which else f"limit {cc.limit_of(nct)}" + ("" if nct == 4 else " only, + named")
        out.append(pytest.param(have, want, id=f"{what}: {len(have & want)} of {len(want)} tiles"))
    return out


@pytest.mark.parametrize("have,want", _coverage())
def test_distinct_tiles_covered(have, want):
    """the count is in the test's id (pytest -v): tiles the table has a row for, of the tiles the sweep returns"""
    assert have == want


def test_epilogue_shapes_are_on_the_tiles_they_claim(ops):
    for F, T, tile, rf, rt in cc.BNR_SHAPES:
        for B in (cc.B_PLAIN, cc.B_XCD):
            p = ops.conv3x3_plan(B, 128, F, T, 128)
            assert (p["TT"], p["FT"]) == tile and (p["nft"] * p["FT"] > F, T % p["TT"] != 0) == (rf, rt) and p["tblocks"] == 2, (F, T, p)
            assert B * T * F * 128 <= cc.MAX_OUT_ELEMS and ops.lib().sed_conv3x3_dgrad_bnred_rows(B, 128, F, T, 128) == p["rows"]
    assert {s[2] for s in cc.BNR_SHAPES} == {(8, 20), (5, 32), (20, 8)} and any(s[3] for s in cc.BNR_SHAPES) and any(s[4] for s in cc.BNR_SHAPES)
    # the pooled inference rows drop a frame where T is odd, and some are
    assert sum(r["T"] % 2 for r in cc.rows(4, 1)) >= 5


def test_the_model_shapes_are_on_the_named_tiles(ops):
    for F, T, tile in [(128, 256, (5, 32)), (40, 256, (8, 20)), (8, 256, (20, 8)), (4, 256, (35, 4))]:
        p = ops.conv3x3_plan(16, 128, F, T, 128)
        assert (p["TT"], p["FT"]) == tile and p["xcd_order"] == 1, (F, T, p)


def test_xcd_remap_is_a_bijection_and_keeps_a_sequence_on_one_xcd():
    grids = {(r["nft"] * r["tblocks"], B) for r in ALL_ROWS for B in (8, 16)} | {(n, 24) for n in (1, 3, 5, 8)}
    for ntiles, B in sorted(grids):
        order = cc.xcd_remap(ntiles, B)
        assert sorted(order) == [(b, t) for b in range(B) for t in range(ntiles)], (ntiles, B)
        for i, (b, t) in enumerate(order):
            assert b % 8 == i % 8                                  # launch index i runs on XCD i % 8: sequence b stays on XCD b % 8
    # off a multiple of 8 the order is the launch order
    assert cc.xcd_remap(3, 3) == [(b, t) for b in range(3) for t in range(3)]
    assert cc.xcd_remap(2, 9)[:3] == [(0, 0), (0, 1), (1, 0)]


def test_stat_row_index_and_tile_slices_partition_the_output():
    for r in ALL_ROWS:
        p = cc.conv_plan(cc.B_XCD, 32, r["F"], r["T"], cc.COUT_OF_NCT[r["nct"]]) if r["which"] == 0 else cc.conv_eval_plan(cc.B_XCD, 32, r["F"], r["T"], 128)
        seen = np.zeros((r["T"], r["F"]), dtype=np.int64)
        idx = []
        for tb in range(p["tblocks"]):
            for fi in range(p["nft"]):
                ts, fs = cc.tile_slices(p, r["F"], r["T"], tb, fi)
                assert ts.stop > ts.start and fs.stop > fs.start, (r["name"], tb, fi)      # no tile without an output position
                seen[ts, fs] += 1
                idx.append(cc.stat_row(p, 2, tb, fi))
        assert (seen == 1).all(), r["name"]
        assert idx == list(range(2 * p["tblocks"] * p["nft"], 3 * p["tblocks"] * p["nft"])), r["name"]


def test_rg_rows_of_the_pooled_table(ops):
    """the shapes the RG test lists (conv_cases.rg_rows) take the fused tap-sum path for both input-channel counts, by the
    library's own answer; the restated condition equals it on every pooled row"""
    L = ops.lib()
    for r in cc.rows(4, 1):
        for B in (cc.B_PLAIN, cc.B_XCD):
            for cin in (1, 2):
                got = L.sed_conv3x3_dgrad_bnred_rg_rows(B, 128, r["F"], r["T"], 128, cin)
                p = cc.conv_plan(B, 128, r["F"], r["T"], 128)
                assert got == (p["rows"] if cc.rg_supported(p, cin) else 0), (r["name"], B, cin)
    listed = cc.rg_rows()
    tiles = {(p["TT"], p["FT"]) for p in (cc.conv_plan(8, 128, r["F"], r["T"], 128) for r in listed)}
    print(f"\nthe tap-sum epilogue runs on {len(listed)} of the {len(cc.rows(4, 1))} pooled rows, on {len(tiles)} distinct conv_plan tiles")
    assert len(listed) >= 40 and len(tiles) >= 40
    for r in listed:
        assert L.sed_conv1_fused_supported(1, r["F"], 2 * r["T"], 128, 1, 2) and L.sed_conv1_fused_supported(2, r["F"], 2 * r["T"], 128, 1, 2)
        for B in (cc.B_PLAIN, cc.B_XCD):
            assert L.sed_conv3x3_dgrad_bnred_rg_rows(B, 128, r["F"], r["T"], 128, 1) > 0 and L.sed_conv3x3_dgrad_bnred_rg_rows(B, 128, r["F"], r["T"], 128, 2) > 0
