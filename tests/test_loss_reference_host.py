"""tests/_loss_reference.py (the float64 references of the loss / metric / optimiser GPU tests) against torch, the oracle and the
committed fixtures.  CPU only."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import maskunet_oracle as O
from tests import _loss_reference as R


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("M,C,Cp,ignore", [(1, 5, 8, 255), (17, 65, 72, 255), (129, 300, 304, -100), (64, 1, 8, -100)])
def test_ce_rows_matches_torch_float64(dtype, M, C, Cp, ignore):
    g = np.random.default_rng(M * 1000 + C)
    x = torch.from_numpy(g.standard_normal((M, Cp)) * 3).to(dtype)
    x[:, C:] = float("nan")                                        # the padding is never read
    if C > 2:
        x[:, 1] = float("-inf")                                    # a -inf logit takes no part
    lab = torch.from_numpy(g.integers(0, C, M))
    lab[lab == 1] = 0
    if M > 1:
        lab[2::5] = ignore
    r = R.ce_rows(x, lab, C, ignore)
    xr = x[:, :C].double().requires_grad_(True)
    ref = F.cross_entropy(xr, lab, ignore_index=ignore)
    ref.backward()
    assert r["count"] == int((lab != ignore).sum())
    assert abs(r["loss"] - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))
    assert np.abs(r["lse"] - torch.logsumexp(xr.detach(), dim=1).numpy()).max() <= 1e-12 * max(1.0, np.abs(r["lse"]).max())
    assert np.abs(r["g"] / r["count"] - xr.grad.numpy()).max() <= 1e-14
    assert np.abs(r["p"] - torch.softmax(xr.detach(), dim=1).numpy()).max() <= 1e-14
    assert np.array_equal(r["mx"], xr.detach().max(dim=1).values.numpy())


def test_ce_rows_every_label_ignored():
    x = torch.randn(9, 8, generator=torch.Generator().manual_seed(1))
    r = R.ce_rows(x, torch.full((9,), 255), 5, 255)
    assert r["count"] == 0 and np.isnan(r["loss"]) and not r["g"].any()
    assert np.isfinite(r["lse"]).all()


def _golden(name):
    return np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))


@pytest.mark.parametrize("name", ["miou_dense", "miou_absent_classes", "miou_ties_150"])
def test_iou_counts_matches_oracle_and_goldens(name):
    g = _golden(name)
    y, t, C = torch.from_numpy(g["y"]), torch.from_numpy(g["t"]), int(g["num_classes"])
    rows = y.permute(0, 2, 3, 1).reshape(-1, C)
    counts, miou = R.iou_counts(rows, t.reshape(-1), C)
    assert abs(miou - float(g["miou"])) <= 1e-7
    assert abs(miou - float(O.mean_iou(y, t, C))) <= 1e-7
    pred = torch.argmax(y, dim=1).reshape(-1)
    for c in range(C):
        assert counts[0, c] == int(((pred == c) & (t.reshape(-1) == c)).sum())
        assert counts[1, c] == int((pred == c).sum()) and counts[2, c] == int((t.reshape(-1) == c).sum())


def test_iou_counts_ties_and_labels_outside_the_classes():
    g = np.random.default_rng(5)
    C, M = 21, 300
    rows = torch.from_numpy(g.integers(0, 8, (M, C)).astype(np.float32) * 0.25)        # 8 distinct values: ties in every row
    t = torch.from_numpy(g.integers(0, C, M))
    t[::9] = 255
    t[4::11] = -1
    counts, miou = R.iou_counts(rows, t, C)
    y = rows.reshape(3, 10, 10, C).permute(0, 3, 1, 2).contiguous()
    assert abs(miou - float(O.mean_iou(y, t.reshape(3, 10, 10), C))) <= 1e-6
    assert counts[1].sum() == M and counts[2].sum() == int(((t >= 0) & (t < C)).sum())
    first = [int(np.flatnonzero(r == r.max())[0]) for r in rows.numpy()]
    assert np.array_equal(counts[1], np.bincount(first, minlength=C))


@pytest.mark.parametrize("eps,scale", [(1e-8, 1.0), (1e-3, 1000.0)])
def test_adamw_steps_matches_torch_float64(eps, scale):
    g = np.random.default_rng(11)
    sizes, wds = [1, 255, 4097], [0.0, 0.1, 0.1]
    lr, betas = 5e-3, (0.9, 0.999)
    p0 = [g.standard_normal(n).astype(np.float32) for n in sizes]
    grads = []
    for it in range(3):
        gs = [g.standard_normal(n).astype(np.float32) for n in sizes]
        for a in gs:
            a[::5] = 0.0
        if it == 1:
            gs[1] = None
        grads.append(gs)
    ours = R.adamw_steps(p0, [[None if a is None else a * np.float32(scale) for a in gs] for gs in grads], lr, betas, eps, wds, scale,
                         set_step={(2, 2): 9998})
    f32 = lambda a: float(np.float32(a))
    tp = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in p0]
    opt = torch.optim.AdamW([{"params": [q], "weight_decay": f32(w)} for q, w in zip(tp, wds)], lr=f32(lr),
                            betas=(f32(betas[0]), f32(betas[1])), eps=f32(eps))
    ginv = f32(1.0 / scale)
    for it, gs in enumerate(grads):
        for i, (q, a) in enumerate(zip(tp, gs)):
            q.grad = None if a is None else torch.from_numpy((a * np.float32(scale)).astype(np.float64) * ginv)
            if (it, i) == (2, 2):
                opt.state[q]["step"] = torch.tensor(9998.0) if torch.is_tensor(opt.state[q]["step"]) else 9998
        opt.step()
        for i, q in enumerate(tp):
            p, m, v, ma = ours[it][i]
            st = opt.state[q]
            assert np.abs(p - q.detach().numpy()).max() <= 1e-13 * max(1.0, np.abs(p).max())
            if st:
                assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-14
                assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-14
                assert np.all(ma >= np.abs(m) - 1e-18)
    assert not ours[2][1][2][::5].any()                            # a gradient that is always 0: v stays 0


@pytest.mark.parametrize("name", ["instloss_ade_small", "instloss_ade_sparse", "instloss_city_ignore", "instloss_none"])
def test_instance_triplet_matches_oracle_and_goldens(name):
    g = _golden(name)
    ign = None if int(g["ignore"]) < 0 else int(g["ignore"])
    mask = g["mask"]
    assert mask.min() >= 0 and mask.max() < 32768                  # all ids in range, and fewer instances than the cap below
    loss, dfeat, hinge = R.instance_triplet(g["feat"], mask, g["u"], 1.0, ign, 32768, 64)
    assert len(hinge) == int(g["draws"])
    assert abs(loss - float(g["loss"])) <= 1e-5                    # the fixture is the reference class in fp32
    assert np.abs(dfeat - g["dfeat"]).max() <= 1e-5
    f = torch.from_numpy(g["feat"]).double().requires_grad_(True)
    ref = O.instance_contrastive_loss(f, torch.from_numpy(mask), torch.from_numpy(g["u"]).double(), 1.0, ign)
    if ref.requires_grad:
        ref.backward()
    assert abs(loss - ref.item()) <= 1e-12
    assert np.abs(dfeat - (f.grad.numpy() if f.grad is not None else 0.0)).max() <= 1e-12


def test_instance_triplet_device_rules():
    """ids outside [0, id_cap) are no instances but stay negatives; the cap keeps the first max_inst ids and divides by that many."""
    g = np.random.default_rng(2)
    feat = g.standard_normal((2, 3, 6, 8))
    mask = np.zeros((2, 6, 8), dtype=np.int64)
    mask[0, 0, :3], mask[0, 2, :2], mask[1, 1, 4:7], mask[1, 5, :2], mask[0, 5, 5:] = 5, 9, 12, 40000, -5
    ids = R.instance_ids(mask, None, 32768, 64)
    assert [i for i, _, _ in ids] == [5, 9, 12] and ids[0][1:] == (3, 93)
    u = [R.u_for_negative(mask, 5, 5 * 8 + 5), R.u_for_negative(mask, 9, 48 + 5 * 8), 0.3]      # negatives: the -5 and the 40000 pixels
    loss, dfeat, hinge = R.instance_triplet(feat, mask, u, 1.0, None, 32768, 64)
    col = lambda b, h: feat[:, :, b, h].reshape(-1)
    d = lambda a, b: np.sqrt(np.sum((a - b + 1e-6) ** 2))
    h0 = d(col(0, 0), col(0, 0)) - d(col(0, 0), col(0, 5)) + 1.0
    h1 = d(col(0, 2), col(0, 2)) - d(col(0, 2), col(1, 5)) + 1.0
    assert abs(hinge[0] - h0) <= 1e-14 and abs(hinge[1] - h1) <= 1e-14
    capped, _, hc = R.instance_triplet(feat, mask, u, 1.0, None, 32768, 2)
    assert len(hc) == 2 and abs(capped - (max(h0, 0.0) + max(h1, 0.0)) / 2) <= 1e-14
    # with every id in range and no cap this is the oracle
    mask2 = np.where((mask < 0) | (mask >= 32768), 0, mask)
    f = torch.from_numpy(feat).requires_grad_(True)
    ref = O.instance_contrastive_loss(f, torch.from_numpy(mask2), torch.tensor(u, dtype=torch.float64), 1.0, None)
    ref.backward()
    l2, d2, _ = R.instance_triplet(feat, mask2, u, 1.0, None, 32768, 64)
    assert abs(l2 - ref.item()) <= 1e-14 and np.abs(d2 - f.grad.numpy()).max() <= 1e-14
    # one id everywhere: no negatives, no instance
    l3, d3, h3 = R.instance_triplet(feat, np.full((2, 6, 8), 3), [0.5], 1.0, None, 32768, 64)
    assert l3 == 0.0 and not d3.any() and len(h3) == 0
