"""CPU: which kernel every convolution shape reaches.  The selection functions of conv.hip are pure host code behind the
mu_conv_*_plan queries (the launches switch on the same functions), so the shape table of the kernel suite can be checked against
them without a GPU: every plan id has a case, the layers of the benchmarked models keep their kernels, the statistics rows agree with
the plan, and both sides of every numeric threshold are cases."""
import collections

import pytest

from tests import _conv_cases as C

# the dtypes in which a plan can be selected at all (from the conditions of the *_pick functions): a NEW plan name must be added here
# and, with a case that reaches it, to tests/_conv_cases.LAYERS
ALL, H, X, HX = ("fp32", "fp16", "fp32x"), ("fp16",), ("fp32x",), ("fp16", "fp32x")
LEGAL = {
    "fwd": {"nt5": H, "nt5_halves": H, "nt4p": H, "nt4": H, "nt4x": X, "nt3_128": ALL, "nt3_64_ring": ALL, "nt3_64": ALL,
            "wide192_sb": H, "wide192": H, "head160_sb": H, "head160": HX, "dma128": ALL, "dma64": ALL,
            # (fp32 / fp32x: Cin % 32 == 0 already makes a row of Cin floats a multiple of 128 bytes -- the LDS-DMA forms take every 64-multiple)
            "gen128": H, "gen64": H, "gen32": ALL},
    "fused": {"nt4f": H, "nt3f_128": ALL, "nt3f_64": ALL, "head160f": H, "dma128f": ALL, "dma64f": ALL, "gen128f": H, "gen64f": H,
              "gen32f": ALL},
    "dgrad_h": {n: X for n in ("nt4hl", "nt3hl_128", "nt3hl_64", "gen128hl", "gen64hl", "gen32hl")},
    # (fp32x column: mu_conv_wgrad_h / mu_conv_wgrad_h1 run the fp16 kernels; the 1x1 layers the wide 160 tile and the generic tiles)
    "wgrad": {"rgb_fma": ("fp32", "fp16"), **{f"rgb2_npt{i}": H for i in range(1, 9)}, **{f"wgrad9_npt{i}": HX for i in range(1, 5)},
              "wgrad9_w16": HX, **{f"wgrad3_{t}{v}": HX for t in ("128", "64") for v in ("_w16", "_rows2", "_flat64", "")},
              "wide192_ci64": H, "wide192_ci128": H, "wide160_ci64": HX, "wide160_ci128": HX,
              "wide192_ci64_bias": H, "wide192_ci128_bias": H, "wide160_ci64_bias": H, "wide160_ci128_bias": H,
              "gen128": ALL, "gen64": ALL, "gen32": ALL},
}
STAT_ROWS = {"nt5": ("t16", 4), "nt4p": ("t16", 4), "nt4": ("t16", 4), "nt4x": ("t16", 4), "nt3_128": ("t8", 2), "nt3_64_ring": ("t8", 4),
             "nt3_64": ("t8", 4)}


def _reach():
    reach = collections.defaultdict(list)
    for c in C.LAYERS:
        for entry, dn, op, pid in C.entries(c):
            assert pid > 0, f"{C.name_of(c)}: {entry} [{dn}] is not served"
            reach[(op, C.plan_name(op, pid), dn)].append(f"{C.name_of(c)}:{entry}")
    return reach


def test_every_plan_name_is_known():
    for op in C.OPS:
        assert sorted(C.all_plan_names(op)) == sorted(LEGAL[op]), op


def test_every_plan_id_is_reached_by_a_case_of_the_table():
    reach = _reach()
    missing = [f"{op}:{name} [{dn}]" for op in C.OPS for name, dts in LEGAL[op].items() for dn in dts if not reach[(op, name, dn)]]
    assert not missing, "kernels without a case in tests/_conv_cases.LAYERS: " + ", ".join(missing)
    stray = [k for k in reach if k[2] not in LEGAL[k[0]][k[1]]]
    assert not stray, f"plans selected in a dtype LEGAL does not list: {stray}"


def test_names_are_stable_and_ids_outside_the_table_have_none():
    from maskunet_amd import _lib
    lib = _lib.load()
    assert C.plan_name("fwd", 1) == "nt5" and C.plan_name("fwd", 8) == "nt3_64"          # the Conv3x3Kernel values
    for op, code in C.OPS.items():
        assert lib.mu_conv_plan_name(code, 0) is None and lib.mu_conv_plan_name(code, lib.mu_conv_plan_count(code)) is None
        names = [lib.mu_conv_plan_name(code, i) for i in range(1, lib.mu_conv_plan_count(code))]
        assert all(names) and len(set(names)) == len(names), (op, names)                   # every id of the table is a reachable kernel
    assert lib.mu_conv_plan_name(7, 1) is None
    # arguments no entry point accepts have no plan
    assert lib.mu_conv_fwd_plan(1, 8, 8, 48, 32, 9, 1, 0) == 0 and lib.mu_conv_fwd_plan(1, 8, 8, 32, 32, 4, 1, 0) == 0
    assert lib.mu_conv_fwd_plan(1, 16, 16, 64, 64, 9, 0, 1) == 0                           # exact fp32 has no statistics epilogue
    assert lib.mu_conv_wgrad_plan(1, 16, 16, 64, 64, 9, 64, 2, 0) == 0                     # fp32x 3x3: mu_conv_wgrad_h / _h1
    assert lib.mu_conv_wgrad_bias_plan(1, 16, 16, 64, 64, 1, 64, 1) == 0


# (B, H = W, Cin, Cout, taps, cin_valid) -> (forward [with statistics where the layer has them], data gradient, weight gradient), fp16:
# every convolution of UNet(3, 150) and InstanceUNet(3, 19, 16) at 128 x 128, B = 64 (the benchmark) and B = 2 (the goldens).
# Written down from the queries; a threshold edit that re-routes a layer shows up as a diff of this table.
MODEL_PLANS = {
    (64, 128, 32, 64, 9, 3): ('gen64', 'gen32', 'rgb2_npt4'),
    (2, 128, 32, 64, 9, 3): ('gen64', 'gen32', 'rgb2_npt4'),
    (64, 128, 64, 64, 9, 64): ('nt5', 'nt5', 'wgrad9_npt4'),
    (2, 128, 64, 64, 9, 64): ('nt3_64', 'nt3_64', 'wgrad9_npt4'),
    (64, 64, 64, 64, 9, 64): ('nt5', 'nt5', 'wgrad9_npt2'),
    (2, 64, 64, 64, 9, 64): ('nt3_64', 'nt3_64', 'wgrad9_npt2'),
    (64, 64, 64, 128, 9, 64): ('nt4p', 'nt3_64_ring', 'wgrad9_npt2'),
    (2, 64, 64, 128, 9, 64): ('nt4', 'nt3_64_ring', 'wgrad9_npt2'),
    (64, 64, 128, 128, 9, 128): ('nt4p', 'nt4p', 'wgrad3_128_flat64'),
    (2, 64, 128, 128, 9, 128): ('nt4', 'nt4', 'wgrad3_128_flat64'),
    (64, 64, 128, 384, 1, 128): ('wide192', 'dma128', 'wide192_ci128'),
    (2, 64, 128, 384, 1, 128): ('wide192', 'dma128', 'wide192_ci128'),
    (64, 32, 128, 128, 9, 128): ('nt4', 'nt4', 'wgrad9_npt1'),
    (2, 32, 128, 128, 9, 128): ('nt4', 'nt4', 'wgrad9_npt1'),
    (64, 32, 128, 256, 9, 128): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (2, 32, 128, 256, 9, 128): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (64, 32, 256, 256, 9, 256): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (2, 32, 256, 256, 9, 256): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (64, 32, 256, 768, 1, 256): ('wide192', 'dma128', 'wide192_ci128'),
    (2, 32, 256, 768, 1, 256): ('wide192', 'dma128', 'wide192_ci128'),
    (64, 16, 256, 256, 9, 256): ('nt4', 'nt4', 'wgrad9_w16'),
    (2, 16, 256, 256, 9, 256): ('nt4', 'nt4', 'wgrad9_w16'),
    (64, 16, 256, 768, 1, 256): ('wide192', 'dma128', 'wide192_ci128'),
    (2, 16, 256, 768, 1, 256): ('wide192', 'dma128', 'wide192_ci128'),
    (64, 16, 256, 512, 9, 256): ('nt4', 'nt4', 'wgrad9_w16'),
    (2, 16, 256, 512, 9, 256): ('nt4', 'nt4', 'wgrad9_w16'),
    (64, 16, 512, 512, 9, 512): ('nt4', 'nt4', 'wgrad9_w16'),
    (2, 16, 512, 512, 9, 512): ('nt4', 'nt4', 'wgrad9_w16'),
    (64, 16, 512, 256, 9, 512): ('nt4', 'nt4', 'wgrad9_w16'),
    (2, 16, 512, 256, 9, 512): ('nt4', 'nt4', 'wgrad9_w16'),
    (64, 32, 512, 512, 9, 512): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (2, 32, 512, 512, 9, 512): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (64, 32, 512, 256, 9, 512): ('nt4', 'nt4p', 'wgrad3_128_rows2'),
    (2, 32, 512, 256, 9, 512): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (64, 32, 256, 128, 9, 256): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (2, 32, 256, 128, 9, 256): ('nt4', 'nt4', 'wgrad3_128_rows2'),
    (64, 32, 128, 384, 1, 128): ('wide192', 'dma128', 'wide192_ci128'),
    (2, 32, 128, 384, 1, 128): ('wide192', 'dma128', 'wide192_ci128'),
    (64, 64, 256, 256, 9, 256): ('nt4p', 'nt4p', 'wgrad3_128_flat64'),
    (2, 64, 256, 256, 9, 256): ('nt4', 'nt4', 'wgrad3_128_flat64'),
    (64, 64, 256, 128, 9, 256): ('nt4p', 'nt4p', 'wgrad3_128_flat64'),
    (2, 64, 256, 128, 9, 256): ('nt4', 'nt4', 'wgrad3_128_flat64'),
    (64, 64, 128, 64, 9, 128): ('nt3_64_ring', 'nt5_halves', 'wgrad9_npt2'),
    (2, 64, 128, 64, 9, 128): ('nt3_64_ring', 'nt4', 'wgrad9_npt2'),
    (64, 64, 64, 192, 1, 64): ('wide192_sb', 'dma64', 'wide192_ci64'),
    (2, 64, 64, 192, 1, 64): ('wide192_sb', 'dma64', 'wide192_ci64'),
    (64, 128, 128, 128, 9, 128): ('nt4p', 'nt4p', 'wgrad3_128_flat64'),
    (2, 128, 128, 128, 9, 128): ('nt4', 'nt4', 'wgrad3_128_flat64'),
    (64, 128, 128, 64, 9, 128): ('nt3_64_ring', 'nt5_halves', 'wgrad9_npt4'),
    (2, 128, 128, 64, 9, 128): ('nt3_64_ring', 'nt4', 'wgrad9_npt4'),
    (64, 128, 64, 192, 1, 64): ('wide192_sb', 'dma64', 'wide192_ci64'),
    (2, 128, 64, 192, 1, 64): ('wide192_sb', 'dma64', 'wide192_ci64'),
    (64, 128, 64, 160, 1, 64): ('head160_sb', 'gen64', 'wide160_ci64'),
    (2, 128, 64, 160, 1, 64): ('head160_sb', 'gen64', 'wide160_ci64'),
    (64, 128, 64, 32, 1, 64): ('gen32', 'gen64', 'gen32'),
    (2, 128, 64, 32, 1, 64): ('gen32', 'gen64', 'gen32'),
    (64, 128, 32, 32, 9, 19): ('gen32', 'gen32', 'gen32'),
    (2, 128, 32, 32, 9, 19): ('gen32', 'gen32', 'gen32'),
    (64, 128, 32, 32, 1, 32): ('gen32', 'gen32', 'gen32'),
    (2, 128, 32, 32, 1, 32): ('gen32', 'gen32', 'gen32'),
}


def test_the_benchmarked_dispatch_is_pinned():
    from maskunet_amd import _lib
    lib = _lib.load()
    seen = set()
    for c_out, three_head in ((150, False), (19, True)):
        layers = C.model_layers(c_out, three_head)
        assert len(layers) == (39 if not three_head else 42), len(layers)      # 32 (35) convolutions + 6 q/k/v projections + the head
        for key, Cin, Cout, taps, cv, hw in layers:
            for B in (64, 2):
                k = (B, hw, Cin, Cout, taps, cv)
                seen.add(k)
                assert k in MODEL_PLANS, f"{key} at B = {B}: {k} has no row in MODEL_PLANS"
                stats = 1 if lib.mu_conv_stats_rows(B, hw, hw, Cin, Cout, taps, 1) else 0
                got = (C.plan_name("fwd", lib.mu_conv_fwd_plan(B, hw, hw, Cin, Cout, taps, 1, stats)),
                       C.plan_name("fwd", lib.mu_conv_fwd_plan(B, hw, hw, Cout, Cin, taps, 1, 0)),
                       C.plan_name("wgrad", lib.mu_conv_wgrad_plan(B, hw, hw, Cin, Cout, taps, cv, 1, 0)))
                assert got == MODEL_PLANS[k], f"{key} at B = {B} {k}: (fwd, dgrad, wgrad) = {got}, pinned {MODEL_PLANS[k]}"
    assert seen == set(MODEL_PLANS)


def test_plan_and_statistics_rows_agree():
    from maskunet_amd import _lib
    lib = _lib.load()
    n = 0
    for c in C.LAYERS:
        B, Hh, W, Cin, Cout, taps = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["taps"]
        for dn, d in C.DTYPES.items():
            rows = lib.mu_conv_stats_rows(B, Hh, W, Cin, Cout, taps, d)
            pid = lib.mu_conv_fwd_plan(B, Hh, W, Cin, Cout, taps, d, 1)
            name = C.plan_name("fwd", pid) if pid else None
            tag = f"{C.name_of(c)} [{dn}]: rows {rows}, plan {name}"
            if taps != 9 or dn == "fp32":
                assert rows == 0 and pid == 0, tag
                continue
            assert (rows > 0) == (name in STAT_ROWS), tag
            if rows:
                unit, per = STAT_ROWS[name]
                tiles = B * (Hh // 16) * (W // 16) if unit == "t16" else B * (Hh // 8) * (W // 16)
                assert rows == per * tiles, tag
                n += 1
    assert n >= 40


@pytest.mark.parametrize("edge", C.EDGES, ids=[e[0] for e in C.EDGES])
def test_both_sides_of_every_threshold_are_cases(edge):
    what, query, dn, below, at = edge
    names = []
    for c in (below, at):
        assert c in C.LAYERS
        got = [C.plan_name(op, pid) for entry, d, op, pid in C.entries(c) if entry == query and d == dn]
        assert len(got) == 1 and got[0], (what, C.name_of(c), got)
        names.append(got[0])
    assert names[0] != names[1], f"{what}: {C.name_of(below)} and {C.name_of(at)} both run {names[0]}"
