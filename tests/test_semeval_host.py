"""CPU: the float64 restatement of the semantic-evaluation contract (tests/_semeval_reference.py) and the host arithmetic of
maskunet_amd.metrics (metrics_from_counts) pinned to the reference-generated fixtures (tests/golden/semeval/*.npz from
make_golden_semeval.py, miou_*.npz from make_golden_losses.py) and to scikit-learn; the argument checks and host-only queries of
mu_sem_eval."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from tests import _semeval_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MU_ERR_ARG, MU_ERR_SHAPE, MU_ERR_WORKSPACE = -1, -2, -4
SEMEVAL_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "semeval", "*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN, "semeval", name + ".npz"))
    y = z["y"].astype(np.float64)
    B, C = y.shape[:2]
    return z, y.transpose(0, 2, 3, 1).reshape(B, -1, C), z["t"].astype(np.int64).reshape(B, -1), int(z["num_classes"])


def updates_of(ref, splits):
    edges = np.cumsum([0] + [int(s) for s in splits])
    return ([ref["img_counts"][a:b] for a, b in zip(edges[:-1], edges[1:])], [ref["img_loss"][a:b] for a, b in zip(edges[:-1], edges[1:])])


def assert_same_metrics(got, ref, tol=1e-12):
    """integers exactly, floats to `tol`; both sides hold the same keys"""
    assert set(got) == set(ref) and set(got["reference"]) == set(ref["reference"])
    worst = 0.0
    for k, r in ref.items():
        if k == "reference":
            continue
        g = got[k]
        if np.asarray(r).dtype.kind in "ib":
            assert np.asarray(g).dtype == np.asarray(r).dtype and np.array_equal(g, r), k
        else:
            assert np.asarray(g).dtype == np.float64 or isinstance(g, float), k
            worst = max(worst, float(np.max(np.abs(np.asarray(g) - np.asarray(r)))))
    for k, r in ref["reference"].items():
        g = got["reference"][k]
        if np.isnan(r):
            assert np.isnan(g), k
        else:
            worst = max(worst, abs(g - r))
    print(f"worst float difference {worst:.3e} (bound {tol:.0e})")
    assert worst <= tol


def test_fixture_set():
    assert SEMEVAL_CASES == ["semeval_absent_classes", "semeval_city19", "semeval_updates_19", "semeval_void_image"]
    for name in SEMEVAL_CASES:
        assert os.path.getsize(os.path.join(GOLDEN, "semeval", name + ".npz")) < 64 * 1024


@pytest.mark.parametrize("name", SEMEVAL_CASES)
def test_restatement_and_host_metrics_match_the_reference_fixtures(name):
    from maskunet_amd import metrics_from_counts
    z, x, t, C = load(name)
    assert (t == 255).any() and t[0, 0] == 0 and t[0, 1] == C - 1
    ref = R.sem_eval(x, t, C, 255)
    per_image = np.array([R.image_iou(c) for c in ref["img_counts"]])
    e_img = np.abs(per_image - z["image_iou"]).max()
    counts, losses = updates_of(ref, z["splits"])
    e_batch = max(abs(R.batch_iou(c) - m) for c, m in zip(counts, z["batch_miou"]))
    print(f"{name}: per-image IoU error {e_img:.3e}, batch mean_iou error {e_batch:.3e} (bound 1e-6)")
    assert e_img <= 1e-6 and e_batch <= 1e-6
    for m in (R.metrics(ref["confusion"], counts, losses), metrics_from_counts(ref["confusion"], counts, losses)):
        assert abs(m["reference"]["image_miou"] - float(z["image_miou"])) <= 1e-6
        assert abs(m["reference"]["batch_miou"] - float(z["batch_miou"].mean())) <= 1e-6
    # the confusion matrix is consistent with the per-image counts by construction
    I, P, L = ref["img_counts"].sum(axis=0)
    assert np.array_equal(ref["confusion"].sum(axis=0), P) and np.array_equal(ref["confusion"][:C].sum(axis=1), L)
    assert np.array_equal(np.diag(ref["confusion"][:C]), I) and ref["confusion"].sum() == t.size
    assert ref["confusion"][C].sum() == (t == 255).sum()


def test_wholly_void_image():
    z, x, t, C = load("semeval_void_image")
    assert (t[1] == 255).all()
    ref = R.sem_eval(x, t, C, 255)
    assert ref["img_loss"][1].tolist() == [0.0, 0.0]
    I, P, L = ref["img_counts"][1]
    assert I.sum() == 0 and L.sum() == 0 and P.sum() == t.shape[1]            # the predictions still enter the unions
    assert 0.0 < z["image_iou"][1] < 1e-6


@pytest.mark.parametrize("name", ["miou_dense", "miou_absent_classes", "miou_ties_150"])
def test_existing_miou_fixtures(name):
    from maskunet_amd import metrics_from_counts
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    y, t, C = z["y"].astype(np.float64), z["t"].astype(np.int64), int(z["num_classes"])
    B = y.shape[0]
    ref = R.sem_eval(y.transpose(0, 2, 3, 1).reshape(B, -1, C), t.reshape(B, -1), C, -100)
    got = metrics_from_counts(ref["confusion"], [ref["img_counts"]], [ref["img_loss"]])["reference"]["batch_miou"]
    err = max(abs(R.batch_iou(ref["img_counts"]) - float(z["miou"])), abs(got - float(z["miou"])))
    print(f"{name}: error {err:.3e} (bound 1e-6)")
    assert err <= 1e-6


def random_counts(C, seed, updates=(2, 1, 3), HW=200, ignore=255):
    rng = np.random.default_rng(seed)
    conf = np.zeros((C + 1, C), np.int64)
    counts, losses = [], []
    for B in updates:
        x = rng.standard_normal((B, HW, C))
        x[:, :, 1] = -50.0                                                     # class 1 is never predicted
        t = rng.integers(0, C - 1, (B, HW))                                    # class C - 1 is never a label: predicted only
        t[t == 2] = 3                                                          # class 2: absent from both sides once its logit is low
        x[:, :, 2] = -50.0
        t[rng.random((B, HW)) < 0.1] = ignore
        r = R.sem_eval(x, t, C, ignore)
        conf += r["confusion"]
        counts.append(r["img_counts"])
        losses.append(r["img_loss"])
    return conf, counts, losses


def test_metrics_from_counts_equals_the_restatement():
    from maskunet_amd import metrics_from_counts
    conf, counts, losses = random_counts(7, 11)
    got, ref = metrics_from_counts(conf, counts, losses, 1e-6), R.metrics(conf, counts, losses, 1e-6)
    assert not ref["present"][2] and ref["support"][1] > 0 and ref["tp"][1] == 0 and ref["support"][6] == 0 and ref["fp"][6] > 0
    assert_same_metrics(got, ref)
    # an update without a counted pixel: its loss is NaN (as torch), and so is the mean over the updates
    losses[1] = np.zeros_like(losses[1])
    got = metrics_from_counts(conf, counts, losses)
    assert np.isnan(got["reference"]["loss"])
    assert_same_metrics(got, R.metrics(conf, counts, losses))


def test_metrics_against_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    from maskunet_amd import metrics_from_counts
    C = 7
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 300, C))
    x[:, :, 1] = -50.0
    x[:, :, 2] = -50.0
    t = rng.integers(0, C - 1, (4, 300))
    t[t == 2] = 3
    t[rng.random(t.shape) < 0.1] = 255
    r = R.sem_eval(x, t, C, 255)
    keep = t.reshape(-1) != 255
    yt, yp = t.reshape(-1)[keep], r["cls"].reshape(-1)[keep]
    worst = 0.0
    for m in (metrics_from_counts(r["confusion"], [r["img_counts"]], [r["img_loss"]]), R.metrics(r["confusion"], [r["img_counts"]], [r["img_loss"]])):
        assert np.array_equal(m["confusion"][:C], sk.confusion_matrix(yt, yp, labels=np.arange(C)))
        pairs = [(m["pixel_accuracy"], sk.accuracy_score(yt, yp))]
        for avg, pre in (("macro", "macro_"), ("weighted", "weighted_")):
            kw = dict(average=avg, zero_division=0)
            pairs += [(m[pre + "precision"], sk.precision_score(yt, yp, **kw)), (m[pre + "recall"], sk.recall_score(yt, yp, **kw)),
                      (m[pre + "f1"], sk.f1_score(yt, yp, **kw)),
                      (m["miou" if avg == "macro" else "weighted_iou"], sk.jaccard_score(yt, yp, **kw))]
        present = m["present"]
        pairs += list(zip(m["iou"][present], sk.jaccard_score(yt, yp, average=None, zero_division=0)))
        worst = max(worst, max(abs(float(a) - float(b)) for a, b in pairs))
    print(f"worst difference to scikit-learn {worst:.3e} (bound 1e-12)")
    assert worst <= 1e-12


def test_invalid_arguments_return_error_codes_without_a_gpu():
    from maskunet_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    nws = lib.mu_sem_eval_workspace_bytes(2, 100, 19)

    def run(**kw):
        a = dict(logits=p, labels=p, B=2, HW=100, C=19, inner=200, outer=0, cs=1, ps=32, ignore=255, inv_t=2.0, counts=p, loss=p,
                 conf=p, cls=None, prob=None, ws=p, nws=nws, dtype=_lib.MU_F16)
        a.update(kw)
        return lib.mu_sem_eval(*a.values(), None)

    for name in ("logits", "labels", "counts", "loss", "conf", "ws"):
        assert run(**{name: None}) == MU_ERR_ARG, name
    assert run(B=0) == MU_ERR_ARG and run(HW=0) == MU_ERR_ARG and run(HW=1 << 31) == MU_ERR_ARG and run(inner=0) == MU_ERR_ARG
    assert run(dtype=2) == MU_ERR_ARG and run(dtype=7) == MU_ERR_ARG
    assert run(inv_t=0.0) == MU_ERR_ARG and run(inv_t=-1.0) == MU_ERR_ARG and run(inv_t=float("nan")) == MU_ERR_ARG
    assert run(C=0) == MU_ERR_SHAPE and run(C=4097) == MU_ERR_SHAPE
    assert run(nws=nws - 1) == MU_ERR_WORKSPACE and run(nws=0) == MU_ERR_WORKSPACE


def test_queries_are_host_only():
    from maskunet_amd import _lib
    lib = _lib.load()
    assert [lib.mu_sem_eval_supported(c) for c in (-1, 0, 1, 150, 4096, 4097)] == [MU_ERR_SHAPE, MU_ERR_SHAPE, 0, 0, 0, MU_ERR_SHAPE]
    assert lib.mu_sem_eval_workspace_bytes(64, 128 * 128, 150) >= 64 * 16
    assert lib.mu_sem_eval_workspace_bytes(1, 1, 1) >= 16 and lib.mu_sem_eval_workspace_bytes(3, 1000, 19) % 16 == 0
    assert lib.mu_sem_eval_workspace_bytes(0, 100, 19) == 0 and lib.mu_sem_eval_workspace_bytes(2, 1 << 31, 19) == 0
    assert lib.mu_sem_eval_workspace_bytes(2, 100, 4097) == 0


def test_lds_crossover_constant_in_step_with_the_header():
    from maskunet_amd import metrics
    src = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "maskunet_hip.h")).read()
    assert int(re.search(r"#define MU_SEM_EVAL_LDS_MAX_C (\d+)", src).group(1)) == metrics.LDS_MAX_CLASSES
    C = metrics.LDS_MAX_CLASSES
    assert ((C + 1) * C + 3 * C) * 4 + 1024 <= 160 * 1024                     # the counters of one workgroup fit a CU's LDS


def test_public_names_and_cpu_tensors_raise():
    import torch
    import maskunet_amd
    for n in ("semantic_eval", "SemanticBatch", "SemanticMetrics", "metrics_from_counts"):
        assert n in maskunet_amd.__all__ and callable(getattr(maskunet_amd, n))
    with pytest.raises(RuntimeError, match="on the GPU"):
        maskunet_amd.semantic_eval(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="before any update"):
        maskunet_amd.SemanticMetrics(3).compute()
