"""tests/_attn_wide_reference.py on the CPU, before tests/test_gpu_attn_wide_edges.py relies on it: every restatement and the whole
block's closed form against float64 torch autograd (1e-10 relative), every input recipe against its own conditions, and teeth -- for
each kernel a list of deliberately wrong restatements, each of which must leave the derived bound on at least one of the very inputs
the GPU file runs, in either storage type."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _attn_wide_reference as R

STORAGES = ("f32", "f16")
SMALL = 4096                          # the teeth run on the cases of at most this many rows (the same recipes as the large ones)


def _close(got, ref, what, rel=1e-10, floor=0.0):
    """max |got - ref| <= rel * max(|ref|_max, floor); `floor` is the size of the terms where the result is a difference of them"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    if ref.size:
        scale = max(float(np.nanmax(np.abs(ref))) if not np.isnan(ref).all() else 0.0, floor, 1e-300)
        err = float(np.nanmax(np.abs(got - ref))) if not np.isnan(ref).all() else 0.0
        assert err <= rel * scale, (what, err, scale)


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).copy())


# ================================================================================================
# parity with torch in float64
# ================================================================================================
def test_gather_scatter_match_torch_indexing():
    for C, ld, rows, cnt in R.gather_cases():
        src, off, idx = R.gather_inputs("f32", C, ld, rows, cnt)
        want = torch.zeros(rows, C, dtype=torch.float32)
        want[:cnt] = torch.from_numpy(src[:, off:off + C])[torch.from_numpy(idx[:cnt]).long()]
        assert R.gather_rows(src[:, off:off + C], idx, cnt, rows).tobytes() == want.numpy().tobytes()
    for C, ld, rows, cnt in R.scatter_cases():
        src, idx = R.scatter_inputs(C, rows, cnt)
        for storage, tt in (("f32", torch.float32), ("f16", torch.float16)):
            val, written = R.scatter_rows(src, idx, cnt, rows, storage)
            if cnt == 0:
                assert written.all() and np.isnan(val.astype(np.float64)).all()
                continue
            want = torch.full((rows, C), -777.0, dtype=tt)
            want[torch.from_numpy(idx[:cnt]).long()] = torch.from_numpy(src[:cnt]).to(tt)          # torch rounds to nearest even
            assert np.array_equal(written, (want != -777.0).any(1).numpy() | written)
            assert val[written].tobytes() == want.numpy()[written].tobytes()
            assert int(written.sum()) == cnt


def test_softmax_and_ds_match_torch_autograd():
    for N, ld, cnt, scale in R.softmax_cases():
        if N > SMALL:
            continue
        s, _ = R.score_rows("f32", N, ld, cnt, scale)
        p, b = R.softmax_rows(s, cnt, scale, "f32")
        assert p.shape == b.shape == (N, ld) and not b[:, cnt:].any()
        if cnt == 0:
            assert np.isnan(p).all()
            continue
        assert not p[:, cnt:].any()
        sc = float(np.float32(scale))
        st_ = _t(s[:, :cnt]).requires_grad_(True)
        pt = torch.softmax(st_ * sc, dim=-1)
        # the same thing as the block states it: a -inf additive key mask over the whole row
        add = torch.zeros(ld, dtype=torch.float64)
        add[cnt:] = -math.inf
        _close(p, torch.softmax(_t(s) * sc + add, dim=-1).numpy(), f"softmax masked {N, ld, cnt}")
        _close(p[:, :cnt], pt.detach().numpy(), f"softmax {N, ld, cnt}")
        d = R.rng(1, N, ld, cnt).standard_normal((N, ld))
        (pt * _t(d[:, :cnt])).sum().backward()
        pf = np.zeros((N, ld))
        pf[:, :cnt] = pt.detach().numpy()
        ds, db = R.attn_wide_ds(pf, d, cnt, scale, "f32")
        _close(ds[:, :cnt], st_.grad.numpy(), f"ds {N, ld, cnt}")
        assert not ds[:, cnt:].any() and not db[:, cnt:].any()
    ds, _ = R.attn_wide_ds(np.ones((2, 4)), np.ones((2, 4)), 0, 1.0, "f32")
    assert np.isnan(ds).all()


def test_layernorm_rows_match_torch_autograd():
    for C, cv, rows in R.ln_cases():
        if rows > SMALL:
            continue
        o, x, g, gamma, beta, _ = R.ln_inputs("f32", C, cv, rows)
        ref = R.ln_rows_fwd(o, x, gamma, beta, cv, R.EPS, "f32")
        v = (_t(o) + _t(x))[:, :cv].clone().requires_grad_(True)
        gm, bt = _t(gamma[:cv]).requires_grad_(True), _t(beta[:cv]).requires_grad_(True)
        eps = float(np.float32(R.EPS))
        y = F.layer_norm(v, (cv,), gm, bt, eps)
        what = f"ln {C, cv, rows}"
        _close(ref["out"][:, :cv], y.detach().numpy(), what + " out")
        assert not ref["out"][:, cv:].any() and not ref["out_b"][:, cv:].any()
        mean = v.detach().mean(1)
        rstd = 1.0 / torch.sqrt(v.detach().var(1, unbiased=False) + eps)
        _close(ref["mean"], mean.numpy(), what + " mean")
        _close(ref["rstd"], rstd.numpy(), what + " rstd")
        (y * _t(g)[:, :cv]).sum().backward()
        bw = R.ln_rows_bwd(g, o, x, ref["mean"], ref["rstd"], gamma, cv, "f32")
        # (a constant or nearly constant row: xhat and the gradient are differences of terms far above their own size)
        terms = float(np.abs(g).max() * np.abs(gamma[:cv]).max() * ref["rstd"].max() * max(1.0, float(np.abs(v.detach().numpy()).max())))
        _close(bw["dY"][:, :cv], v.grad.numpy(), what + " dY", floor=terms * float(ref["rstd"].max()))
        _close(bw["gxh"][:, :cv].sum(0), gm.grad.numpy(), what + " dgamma", floor=terms)
        _close(g.astype(np.float64)[:, :cv].sum(0), bt.grad.numpy(), what + " dbeta")
        assert not bw["dY"][:, cv:].any() and not bw["gxh"][:, cv:].any() and not bw["dY_b"][:, cv:].any()


def _torch_block(case):
    """the block from torch.softmax / F.layer_norm with a -inf additive key mask, float64 autograd"""
    B, N, cv = case["B"], case["N"], case["cv"]
    x = _t(case["x"]).requires_grad_(True)
    p = {k: _t(case[k]).requires_grad_(True) for k in ("wq", "bq", "wk", "bk", "wv", "bv", "gamma", "beta")}
    add = torch.full((B, 1, N), -math.inf, dtype=torch.float64)
    for b in range(B):
        add[b, 0, torch.from_numpy(case["kidx"][b, :case["kcnt"][b]]).long()] = 0.0
    Q, K, V = F.linear(x, p["wq"], p["bq"]), F.linear(x, p["wk"], p["bk"]), F.linear(x, p["wv"], p["bv"])
    Q.retain_grad(), K.retain_grad(), V.retain_grad()
    attn = torch.softmax(Q @ K.transpose(-2, -1) / math.sqrt(cv) + add, dim=-1)
    out = F.layer_norm(attn @ V + x, (cv,), p["gamma"], p["beta"], float(np.float32(R.EPS)))
    (out * _t(case["gout"])).sum().backward()
    res = {"out": out.detach(), "dx": x.grad, "dq": Q.grad, "dk": K.grad, "dv": V.grad}
    res.update({"d" + k: v.grad for k, v in p.items()})
    return {k: v.numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", R.BLOCK_CASES)
def test_block_closed_form_matches_torch_autograd(name):
    case = R.block_case(name, "f32")
    ref, want = R.block_ref(case), _torch_block(case)
    for k in ("out", "dx", "dwq", "dbq", "dwk", "dwv", "dbv", "dgamma", "dbeta", "dq", "dk", "dv"):
        _close(ref[k], want[k], f"block {name} {k}")
    # key.bias: analytically zero (softmax shift invariance) -- both are rounding noise of sums of this size
    size = float(np.abs(ref["dbq"]).max())
    assert float(np.abs(ref["dbk"]).max()) <= 1e-10 * size and float(np.abs(want["dbk"]).max()) <= 1e-10 * size


# ================================================================================================
# the recipes meet their own conditions
# ================================================================================================
@pytest.mark.parametrize("storage", STORAGES)
def test_recipes_meet_their_conditions(storage):
    for C, ld, rows, cnt in R.gather_cases():
        src, off, idx = R.gather_inputs(storage, C, ld, rows, cnt)
        assert src.shape == (rows, ld) and 0 <= cnt <= rows and off + C <= ld
        assert R.representable(src[:, off:off + C], storage)
        assert np.isnan(src.astype(np.float64)).sum() == rows * (ld - C)          # the columns around are poison
        assert sorted(idx.tolist()) == list(range(rows)) and idx.dtype == np.int32
    for C, ld, rows, cnt in R.scatter_cases():
        src, idx = R.scatter_inputs(C, rows, cnt)
        assert src.dtype == np.float32 and np.isfinite(src).all() and np.isfinite(src.astype(np.float16)).all()
        assert 0 <= cnt <= rows and sorted(idx.tolist()) == list(range(rows))
        if C >= 3:                                               # the ties: halfway between two fp16 neighbours, to even
            assert src[0, :3].astype(np.float16).tolist() == [1.0, 1.0 + 2.0 ** -9, -2.0]
    seen = set()
    for N, ld, cnt, scale in R.softmax_cases():
        s, names = R.score_rows(storage, N, ld, cnt, scale)
        assert s.shape == (N, ld) and 0 <= cnt <= ld and R.representable(s, storage)
        p, d, _ = R.ds_inputs(storage, N, ld, cnt, scale)
        assert R.representable(p, storage) and R.representable(d, storage) and p.shape == d.shape == (N, ld)
        assert (p.astype(np.float64)[:, cnt:] > 0.04).all()                       # garbage behind cnt, not zeros
        sc = float(np.float32(scale))
        for r, nm in enumerate(names[:5]):
            seen.add(nm)
            if cnt < 2:
                continue
            x = sc * (s[r, :cnt].astype(np.float64) - float(s[r, :cnt].max()))
            if nm == "constant":
                assert not x.any()
            elif nm == "dominant":                                                # all other probabilities underflow, in fp32 too
                assert np.sort(x)[-2] < -110.0 and math.exp(np.sort(x)[-2]) < 2.0 ** -149 and abs(sc * float(s[r, :cnt].max())) < 130
            elif nm == "span80":
                assert 76.0 <= -x.min() <= 84.0
    assert seen == set(R.SCORE_RECIPES)
    seen = set()
    for C, cv, rows in R.ln_cases():
        o, x, g, gamma, beta, names = R.ln_inputs(storage, C, cv, rows)
        assert o.shape == x.shape == g.shape == (rows, C) and 1 <= cv <= C
        assert all(R.representable(a, storage) for a in (o, x, g)) and gamma.dtype == beta.dtype == np.float32
        v = (o.astype(np.float64) + x.astype(np.float64))[:, :cv]
        for r, nm in enumerate(names[:4]):
            seen.add(nm)
            if nm == "constant":
                assert (v[r] == 1.75).all()
            elif nm == "mean100" and cv >= 24:
                assert abs(v[r].mean() - 100.0) < 0.01 and 0.005 < v[r].std() < 0.02
    assert seen == set(R.LN_RECIPES) and (1, 1) in R.LN_SHAPES
    for name in R.BLOCK_CASES:
        case = R.block_case(name, storage)
        B, N, cv = case["B"], case["N"], case["cv"]
        assert B <= 3 and N <= 272 and N == case["H"] * case["W"] and cv > 256
        assert R.representable(case["x"], storage) and R.representable(case["gout"], storage)
        kidx, kcnt = case["kidx"], case["kcnt"]
        assert kidx.dtype == kcnt.dtype == np.int32 and (kidx >= 0).all() and (kidx < N).all() and (kcnt >= 1).all()
        for b in range(B):
            kept = kidx[b, :kcnt[b]].tolist()
            assert len(set(kept)) == len(kept) <= kidx.shape[1]
        worst = max(float(np.abs(s).max()) for s in R.raw_scores(case))
        assert worst < 65504.0
        if name == "short_list":
            assert kidx.shape[1] == 20 < N and kept != sorted(kept)
        elif name == "n272":
            assert N == 272 and kcnt[0] > 256
        elif name == "cv520":
            assert cv == 520
        elif name == "stale":
            assert kcnt.tolist()[:2] == [N, 1]
        elif name == "dominant":
            s = R.raw_scores(case)[0]
            col = kcnt[0] and int(np.argmax(s[0]))
            assert worst <= R.QK_CAP and (np.argmax(s, 1) == col).all() and 150.0 < float(s[:, col].min())
            assert float(np.delete(s, col, 1).max()) < 60.0


# ================================================================================================
# teeth
# ================================================================================================
def _leaves(mut, ref, bound):
    """the wrong restatement leaves the bound somewhere (a NaN on one side only counts)"""
    mut, ref = np.asarray(mut, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nm, nr = np.isnan(mut), np.isnan(ref)
    with np.errstate(invalid="ignore"):
        return bool((nm != nr).any() or (np.abs(mut - ref)[~nm & ~nr] > np.broadcast_to(bound, ref.shape)[~nm & ~nr]).any())


def _softmax_mutant(kind, s, cnt, ld, scale, storage):
    if kind == "cnt+1":
        if cnt >= ld:
            return None
        m = R.softmax_rows(s, cnt + 1, scale, storage)[0]
        m[:, cnt] = 0.0
        return m
    if kind == "ld":
        return R.softmax_rows(s, ld, scale, storage)[0]
    if kind == "drop_last":
        return R.softmax_rows(s, cnt - 1, scale, storage)[0] if cnt else None
    return R.softmax_rows(s, cnt, {"scale_twice": scale * scale, "scale_missing": 1.0}[kind], storage)[0]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kind", ["cnt+1", "ld", "drop_last", "scale_twice", "scale_missing"])
def test_teeth_softmax(kind, storage):
    caught = 0
    for N, ld, cnt, scale in R.softmax_cases():
        s, _ = R.score_rows(storage, N, ld, cnt, scale)
        mut = _softmax_mutant(kind, s, cnt, ld, scale, storage)
        if mut is not None:
            caught += _leaves(mut, *R.softmax_rows(s, cnt, scale, storage))
    assert caught, kind


def _ds_mutant(kind, p, d, cnt, ld, scale, storage):
    p64, d64, sc = p.astype(np.float64), d.astype(np.float64), float(np.float32(scale))
    if kind == "cnt+1":
        if cnt >= ld or cnt == 0:
            return None
        a = (p64[:, :cnt + 1] * d64[:, :cnt + 1]).sum(1, keepdims=True) / p64[:, :cnt + 1].sum(1, keepdims=True)
        m = np.zeros(p64.shape)
        m[:, :cnt] = p64[:, :cnt] * (d64[:, :cnt] - a) * sc
        return m
    if kind == "ld":
        return R.attn_wide_ds(p, d, ld, scale, storage)[0]
    if kind == "drop_last":
        return R.attn_wide_ds(p, d, cnt - 1, scale, storage)[0] if cnt else None
    if kind == "a_missing":
        if cnt == 0:
            return None
        m = np.zeros(p64.shape)
        m[:, :cnt] = p64[:, :cnt] * d64[:, :cnt] * sc
        return m
    return R.attn_wide_ds(p, d, cnt, {"scale_twice": scale * scale, "scale_missing": 1.0}[kind], storage)[0]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kind", ["cnt+1", "ld", "drop_last", "scale_twice", "scale_missing", "a_missing"])
def test_teeth_ds(kind, storage):
    caught = 0
    for N, ld, cnt, scale in R.softmax_cases():
        p, d, _ = R.ds_inputs(storage, N, ld, cnt, scale)
        mut = _ds_mutant(kind, p, d, cnt, ld, scale, storage)
        if mut is not None:
            caught += _leaves(mut, *R.attn_wide_ds(p, d, cnt, scale, storage))
    assert caught, kind


def test_teeth_ds_row_sum_missing():
    """a = sum p d without the division by sum p: the same thing for an exact softmax row, but not for one stored in fp16 (its sum is
    off 1 by up to half an fp16 ulp of the largest entry) -- the kernel-level bound tells the two apart"""
    caught = 0
    for N, ld, cnt, scale in R.softmax_cases():
        if cnt:
            p, d, _ = R.ds_inputs("f16", N, ld, cnt, scale)
            p64, d64 = p.astype(np.float64)[:, :cnt], d.astype(np.float64)[:, :cnt]
            mut = np.zeros(p.shape)
            mut[:, :cnt] = p64 * (d64 - (p64 * d64).sum(1, keepdims=True)) * float(np.float32(scale))
            caught += _leaves(mut, *R.attn_wide_ds(p, d, cnt, scale, "f16"))
    assert caught


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kind", ["mean_over_C", "eps_omitted", "pad_not_zeroed"])
def test_teeth_ln_fwd(kind, storage):
    caught = {"out": 0, "mean": 0, "rstd": 0}
    for C, cv, rows in R.ln_cases():
        o, x, g, gamma, beta, _ = R.ln_inputs(storage, C, cv, rows)
        ref = R.ln_rows_fwd(o, x, gamma, beta, cv, R.EPS, storage)
        with np.errstate(divide="ignore", invalid="ignore"):
            if kind == "mean_over_C":
                mut = R.ln_rows_fwd(o, x, gamma, beta, C, R.EPS, storage)
                mut["out"][:, cv:] = 0.0
            elif kind == "eps_omitted":
                mut = R.ln_rows_fwd(o, x, gamma, beta, cv, 0.0, storage)
            else:
                mut = dict(ref, out=ref["out"].copy())
                mut["out"][:, cv:] = beta[cv:]
        for k in caught:
            caught[k] += _leaves(mut[k], ref[k], ref[k + "_b"])
    assert caught["out"], kind
    if kind != "pad_not_zeroed":
        assert caught["rstd"] and (kind == "eps_omitted" or caught["mean"]), (kind, caught)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kind", ["mean_over_C", "pad_not_zeroed", "dgamma_dbeta_swapped"])
def test_teeth_ln_bwd(kind, storage):
    caught = {"dY": 0, "gxh": 0}
    for C, cv, rows in R.ln_cases():
        o, x, g, gamma, beta, _ = R.ln_inputs(storage, C, cv, rows)
        f = R.ln_rows_fwd(o, x, gamma, beta, cv, R.EPS, storage)
        mean, rstd = f["mean"].astype(np.float32), f["rstd"].astype(np.float32)
        ref = R.ln_rows_bwd(g, o, x, mean, rstd, gamma, cv, storage)
        if kind == "mean_over_C":
            mut = R.ln_rows_bwd(g, o, x, mean, rstd, gamma, C, storage)
            mut["dY"][:, cv:], mut["gxh"][:, cv:] = 0.0, 0.0
        elif kind == "pad_not_zeroed":
            mut = {k: ref[k].copy() for k in caught}
            mut["dY"][:, cv:], mut["gxh"][:, cv:] = (g.astype(np.float64) * gamma)[:, cv:], g.astype(np.float64)[:, cv:]
        else:                                       # what is summed into dgamma is dbeta's operand
            mut = dict(dY=ref["dY"], gxh=np.where(np.arange(C) < cv, g.astype(np.float64), 0.0))
        for k in caught:
            caught[k] += _leaves(mut[k], ref[k], ref[k + "_b"])
    assert caught["gxh"] if kind == "dgamma_dbeta_swapped" else (caught["dY"] and (kind == "mean_over_C" or caught["gxh"])), (kind, caught)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kind", ["idx_as_j", "cnt+1", "ld", "drop_last"])
def test_teeth_gather_scatter(kind, storage):
    """bound 0: a wrong restatement is caught wherever a single byte differs"""
    caught = 0
    for C, ld, rows, cnt in R.gather_cases():
        src, off, idx = R.gather_inputs(storage, C, ld, rows, cnt)
        body = src[:, off:off + C]
        ref = R.gather_rows(body, idx, cnt, rows)
        use_idx = np.arange(rows, dtype=np.int32) if kind == "idx_as_j" else idx
        use_cnt = {"idx_as_j": cnt, "cnt+1": min(cnt + 1, rows), "ld": rows, "drop_last": max(cnt - 1, 0)}[kind]
        caught += R.gather_rows(body, use_idx, use_cnt, rows).tobytes() != ref.tobytes()
    assert caught, ("gather", kind)
    if kind == "ld":
        return                                      # the scatter has no tail rule: it touches the listed rows only
    caught = 0
    for C, ld, rows, cnt in R.scatter_cases():
        src, idx = R.scatter_inputs(C, rows, cnt)
        val, written = R.scatter_rows(src, idx, cnt, rows, storage)
        use_idx = np.arange(rows, dtype=np.int32) if kind == "idx_as_j" else idx
        use_cnt = {"idx_as_j": cnt, "cnt+1": min(cnt + 1, rows), "drop_last": max(cnt - 1, 0)}[kind]
        mval, mwritten = R.scatter_rows(src, use_idx, use_cnt, rows, storage)
        caught += (not np.array_equal(written, mwritten)) or val[written].tobytes() != mval[written].tobytes()
    assert caught, ("scatter", kind)


@pytest.mark.parametrize("storage,tol", [("f32", 1e-3), ("f16", 3e-2)])
def test_teeth_block_gate(storage, tol):
    """the block-level gate (max error over the reference's max, at the project's tolerances) against wrong closed forms: dgamma and
    dbeta swapped, the scale missing or applied twice, the last kept key dropped"""
    rel = lambda got, ref: float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-12)      # noqa: E731
    case = R.block_case("short_list", storage)
    ref = R.block_ref(case)
    assert rel(ref["dbeta"], ref["dgamma"]) > tol and rel(ref["dgamma"], ref["dbeta"]) > tol
    dropped = dict(case, kcnt=case["kcnt"] - 1)
    assert rel(R.block_ref(dropped)["out"], ref["out"]) > tol
    for factor in (math.sqrt(case["cv"]), 1.0 / math.sqrt(case["cv"])):      # scale missing / twice: fold it into the query projection
        mut = R.block_ref(dict(case, wq=case["wq"] * np.float32(factor), bq=case["bq"] * np.float32(factor)))
        assert rel(mut["out"], ref["out"]) > tol
