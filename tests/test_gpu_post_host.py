"""The host layer of the post-processing entry points that take a workspace (maskunet_amd/csrc/instances.hip, rle.hip, panoptic.hip,
semeval.hip, semeval_native.hip, pil_resize.hip): that the size a `mu_*_workspace_bytes` query states and the regions the launcher
carves are one statement, what each entry refuses and with which code, and that a refused call enqueues nothing.  What the kernels
compute is the business of the test files of each entry point, not of this one.

Every tensor operand sits in a tests/_device_buffers.Guarded buffer and every call goes through _lib.call: after each call the guard bands
are intact and the inputs byte-identical; after a refused call every output still holds its sentinel.

Per entry point and shape (B = 2 images throughout, so that region-major layouts differ from image-major ones):
  exact workspace   a call with exactly the queried bytes between guard bands, and one with a larger, sentinel-filled workspace, give
                    byte-identical outputs, and the larger one's bytes past the query still hold the sentinel;
  short workspace   ws_bytes = query - 1 is MU_ERR_WORKSPACE (mu_pil_resize_u8_nhwc: MU_ERR_ARG, its documented convention);
  refusals          a null pointer and an unknown dtype / kind are MU_ERR_ARG, a limit + 1 (or a lower bound - 1) is MU_ERR_SHAPE.
Refusal order (include/maskunet_hip.h): arguments, limits, workspace, the LDS grant -- which cannot be made to fail on a GPU and is the
business of tools/post_host_launches.cpp -- and only then the first kernel or memset."""
import ctypes

import numpy as np
import pytest
import torch

from tests._device_buffers import Guarded

pytestmark = pytest.mark.gpu

MU_F32, BAD = 0, 7
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
ARG, SHAPE, WORKSPACE = "MU_ERR_ARG", "MU_ERR_SHAPE", "MU_ERR_WORKSPACE"
B, NC, CAP, D, K, T, A = 2, 3, 4, 5, 5, 2, 2
EXTRA = 4096                                      # bytes of the larger workspace past the query
# H, W, max_inst (also max_seg, max_id and both max_inst_* of the match entries), C of the semantic sweeps
SHAPES = {"7x9-m5-c5": (7, 9, 5, 5), "8x8-m8-c40": (8, 8, 8, 40)}
RAGGED = ((11, 13), (6, 20))                      # the label / image sizes of the two ragged batches


class Host:
    """a host array an entry point reads during the call (thr, area_rng)"""

    def __init__(self, values):
        self.a = np.ascontiguousarray(values, dtype=np.float64)

    @property
    def p(self):
        return self.a.ctypes.data_as(ctypes.c_void_p)


class Spec:
    """one entry point at one shape: `order` = the argument names in signature order (without the stream), `ins` = the inputs and
    scalars by name, `outs` = name -> (elements, dtype), `query` = the size query's name and arguments, `short` = the code of a short
    workspace, `refusals` = (label, code, overrides); an override that is callable gets the argument dict"""

    def __init__(self, entry, order, ins, outs, query, refusals, short=WORKSPACE):
        self.entry, self.order, self.ins, self.outs, self.query, self.refusals, self.short = entry, order, ins, outs, query, refusals, short

    def fresh_outs(self):
        return {k: Guarded(n, dt, name=k) for k, (n, dt) in self.outs.items()}

    def ws_query(self):
        from maskunet_amd import _lib
        return int(getattr(_lib.load(), self.query[0])(*self.query[1:]))


def _raw(a):
    return a.p if isinstance(a, (Guarded, Host)) else a


def _args(spec, outs, ws, ws_bytes, over=()):
    v = dict(spec.ins, **outs, ws=ws, ws_bytes=ws_bytes)
    for k, x in dict(over).items():
        v[k] = x(v) if callable(x) else x
    return [v[k] for k in spec.order]


def _guards(args):
    for a in args:
        if isinstance(a, Guarded):
            a.check()


def _call(entry, args):
    from maskunet_amd import _lib
    _lib.call(entry, *[_raw(a) for a in args], _lib.stream())
    torch.cuda.synchronize()
    _guards(args)


def _refused(code, spec, outs, ws, ws_bytes, over=()):
    """`code` before anything is enqueued: after a synchronise every output still holds the sentinel"""
    from maskunet_amd import _lib
    args = _args(spec, outs, ws, ws_bytes, over)
    with pytest.raises(RuntimeError, match=code):
        _lib.call(spec.entry, *[_raw(a) for a in args], _lib.stream())
    torch.cuda.synchronize()
    _guards(args + list(outs.values()))
    for o in outs.values():
        assert bool((o.t == o.sent).all()), (spec.entry, code, o.name, "written by a refused call")


def _run(spec, ws_bytes):
    outs, ws = spec.fresh_outs(), Guarded(ws_bytes, U8, name="ws")
    _call(spec.entry, _args(spec, outs, ws, ws_bytes))
    return outs, ws


# ================================================================================================
# inputs: made once per shape and shared; the match and panoptic entries read what mu_instances and mu_instance_pairs wrote
# ================================================================================================
INST_OUTS = lambda N, M: {"ids": (B * N, I32), "table": (B * M * 8, I32), "score": (B * M, F32), "count": (B, I32), "order": (B * M, I32)}
INST_TAIL = ("ids", "table", "score", "count", "order", "ws", "ws_bytes")
_CACHE = {}


def _ragged(rng, channels, high):
    """a ragged uint8 batch of RAGGED: bytes, offsets int64 [B+1], sizes int32 [B,2]"""
    sizes = np.array(RAGGED, dtype=np.int32)
    lens = sizes[:, 0] * sizes[:, 1] * channels
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.integers(0, high, size=int(offsets[-1])).astype(np.uint8), offsets, sizes


def _instances_spec(name, cls, prob):
    H, W, M, _ = SHAPES[name]
    ins = {"cls": Guarded(B * H * W, I32, data=cls, name="cls"), "prob": Guarded(B * H * W, F32, data=prob, name="prob"), "B": B, "H": H,
           "W": W, "max_inst": M}
    return Spec("mu_instances", ("cls", "prob", "B", "H", "W", "max_inst") + INST_TAIL, ins, INST_OUTS(H * W, M),
                ("mu_instances_workspace_bytes", B, H, W, M),
                [("null cls", ARG, {"cls": None}), ("max_inst 4097", SHAPE, {"max_inst": 4097}), ("max_inst 0", SHAPE, {"max_inst": 0}),
                 ("H * W 65537", SHAPE, {"H": 1, "W": 65537})])


def _chain(name):
    """predicted and ground-truth instances of two random class maps and their pair table, as the device wrote them"""
    if name not in _CACHE:
        H, W, M, _ = SHAPES[name]
        rng = np.random.default_rng(len(name))
        side = {}
        for who in ("pred", "gt"):
            cls = rng.integers(0, NC, size=(B, H, W)).astype(np.int32)
            spec = _instances_spec(name, cls, rng.random((B, H, W), dtype=np.float32))
            outs, _ = _run(spec, spec.ws_query())
            side[who] = dict({k: o.host() for k, o in outs.items()}, cls=cls.reshape(-1))
        spec = _pairs_spec(name, side["pred"]["ids"], side["gt"]["ids"])
        outs, _ = _run(spec, spec.ws_query())
        side["pairs"] = {k: o.host() for k, o in outs.items()}
        _CACHE[name] = side
    return _CACHE[name]


def _pairs_spec(name, pred_ids, gt_ids):
    H, W, M, _ = SHAPES[name]
    ins = {"pred_ids": Guarded(B * H * W, I32, data=pred_ids, name="pred_ids"), "gt_ids": Guarded(B * H * W, I32, data=gt_ids, name="gt_ids"),
           "B": B, "H": H, "W": W, "mp": M, "mg": M}
    return Spec("mu_instance_pairs", ("pred_ids", "gt_ids", "B", "H", "W", "mp", "mg", "pairs", "n_pairs", "ws", "ws_bytes"), ins,
                {"pairs": (B * H * W * 3, I32), "n_pairs": (B, I32)}, ("mu_instance_pairs_workspace_bytes", B, H, W, M, M),
                [("null gt_ids", ARG, {"gt_ids": None}), ("max_inst_pred 4097", SHAPE, {"mp": 4097}), ("max_inst_gt 0", SHAPE, {"mg": 0})])


def _match_ins(name):
    H, W, M, _ = SHAPES[name]
    c = _chain(name)
    g = lambda key, n, dt, data: Guarded(n, dt, data=data, name=key)
    return {"pairs": g("pairs", B * H * W * 3, I32, c["pairs"]["pairs"]), "n_pairs": g("n_pairs", B, I32, c["pairs"]["n_pairs"]),
            "ptable": g("ptable", B * M * 8, I32, c["pred"]["table"]), "pscore": g("pscore", B * M, F32, c["pred"]["score"]),
            "porder": g("porder", B * M, I32, c["pred"]["order"]), "pcount": g("pcount", B, I32, c["pred"]["count"]),
            "gtable": g("gtable", B * M * 8, I32, c["gt"]["table"]), "gcount": g("gcount", B, I32, c["gt"]["count"]),
            "B": B, "H": H, "W": W, "mp": M, "mg": M, "nc": NC, "K": K, "max_dets": 100, "thr": Host([0.5, 0.75]), "T": T}


MATCH_REFUSALS = [("null pairs", ARG, {"pairs": None}), ("T 33", SHAPE, {"T": 33}), ("K max_inst_pred + 1", SHAPE, {"K": lambda v: v["mp"] + 1}),
                  ("num_classes 1025", SHAPE, {"nc": 1025}), ("a threshold of 0", ARG, {"thr": Host([0.5, 0.0])})]


def _match_spec(name):
    order = ("pairs", "n_pairs", "ptable", "pscore", "porder", "pcount", "gtable", "gcount", "B", "H", "W", "mp", "mg", "nc", "K", "max_dets",
             "thr", "T", "det_valid", "det_class", "det_score", "det_gt", "det_iou", "gt_per_class", "pq_gt", "pq_iou", "pq_fp", "overflow",
             "ws", "ws_bytes")
    outs = {"det_valid": (B * K, I32), "det_class": (B * K, I32), "det_score": (B * K, F32), "det_gt": (B * T * K, I32),
            "det_iou": (B * T * K, F64), "gt_per_class": (B * NC, I32), "pq_gt": (B * K, I32), "pq_iou": (B * K, F64), "pq_fp": (B * K, I32),
            "overflow": (B, I32)}
    return Spec("mu_instance_match", order, _match_ins(name), outs, ("mu_instance_match_workspace_bytes", B, K), MATCH_REFUSALS)


def _coco_match_spec(name):
    M = SHAPES[name][2]
    rng = np.random.default_rng(7)
    ins = dict(_match_ins(name), gcrowd=Guarded(B * M, I32, data=rng.integers(0, 2, size=B * M), name="gcrowd"), garea=None,
               rng=Host([[0.0, 1e10], [0.0, 16.0]]), A=A)
    order = ("pairs", "n_pairs", "ptable", "pscore", "porder", "pcount", "gtable", "gcount", "gcrowd", "garea", "B", "H", "W", "mp", "mg", "nc",
             "K", "max_dets", "thr", "T", "rng", "A", "det_valid", "det_class", "det_rank", "det_score", "det_gt", "det_iou", "det_ignore",
             "gt_counted", "pq_gt_per_class", "pq_gt", "pq_iou", "pq_fp", "overflow", "ws", "ws_bytes")
    outs = {"det_valid": (B * K, I32), "det_class": (B * K, I32), "det_rank": (B * K, I32), "det_score": (B * K, F32),
            "det_gt": (B * A * T * K, I32), "det_iou": (B * A * T * K, F64), "det_ignore": (B * A * T * K, U8), "gt_counted": (B * A * NC, I32),
            "pq_gt_per_class": (B * NC, I32), "pq_gt": (B * K, I32), "pq_iou": (B * K, F64), "pq_fp": (B * K, I32), "overflow": (B, I32)}
    return Spec("mu_coco_match", order, ins, outs, ("mu_coco_match_workspace_bytes", B, K),
                MATCH_REFUSALS + [("A 5", SHAPE, {"A": 5}), ("an inverted area range", ARG, {"rng": Host([[0.0, 1e10], [9.0, 4.0]])})])


def _dbscan_spec(name):
    H, W, M, _ = SHAPES[name]
    rng = np.random.default_rng(11)
    N = H * W
    ins = {"cls": Guarded(B * N, I32, data=rng.integers(0, NC, size=B * N), name="cls"),
           "emb": Guarded(B * D * N, F32, data=rng.integers(0, 3, size=B * D * N).astype(np.float32), name="emb"),        # NCHW
           "B": B, "H": H, "W": W, "D": D, "inner": N, "outer": D * N, "cs": N, "ps": 1, "dtype": MU_F32, "nc": NC, "eps": 0.5,
           "min_samples": 2, "max_inst": M}
    order = ("cls", "emb", "B", "H", "W", "D", "inner", "outer", "cs", "ps", "dtype", "nc", "eps", "min_samples", "max_inst") + INST_TAIL
    return Spec("mu_dbscan_instances", order, ins, INST_OUTS(N, M), ("mu_dbscan_workspace_bytes", B, H, W, NC, M),
                [("null emb", ARG, {"emb": None}), ("dtype", ARG, {"dtype": BAD}), ("D 65", SHAPE, {"D": 65}),
                 ("num_classes 1025", SHAPE, {"nc": 1025}), ("B 65536", SHAPE, {"B": 65536})])


def _idmap_spec(name):
    H, W, M, _ = SHAPES[name]
    rng = np.random.default_rng(13)
    N = H * W
    ins = {"id_map": Guarded(B * N, I32, data=rng.choice([0, 3, 26001, 26002, 33000, -5, 7, 900], size=B * N), name="id_map"),
           "kind": 0, "sem": Guarded(B * N, I32, data=rng.integers(0, CAP, size=B * N), name="sem"), "B": B, "H": H, "W": W, "max_inst": M,
           "class_cap": CAP}
    order = ("id_map", "kind", "sem", "B", "H", "W", "max_inst", "class_cap", "ids", "table", "score", "count", "order", "values", "invalid",
             "ws", "ws_bytes")
    return Spec("mu_id_instances", order, ins, dict(INST_OUTS(N, M), values=(B * M, I32), invalid=(B, I32)),
                ("mu_id_instances_workspace_bytes", B, H, W, M, CAP),
                [("null sem", ARG, {"sem": None}), ("kind", ARG, {"kind": BAD}), ("class_cap 1025", SHAPE, {"class_cap": 1025}),
                 ("class_cap 0", SHAPE, {"class_cap": 0})])


def _rle_spec(name):
    H, W, M, _ = SHAPES[name]
    N, L = H * W, 2 * H * W + K
    ins = {"ids": Guarded(B * N, I32, data=_chain(name)["pred"]["ids"], name="ids"),
           "sel": Guarded(B * K, I32, data=np.tile(np.arange(1, K + 1, dtype=np.int32), B), name="sel"), "B": B, "H": H, "W": W, "K": K, "max_id": M}
    order = ("ids", "sel", "B", "H", "W", "K", "max_id", "offsets", "counts", "area", "str_offsets", "str_bytes", "ws", "ws_bytes")
    outs = {"offsets": (B * (K + 1), I32), "counts": (B * L, I32), "area": (B * K, I32), "str_offsets": (B * (K + 1), I32),
            "str_bytes": (B * 4 * L, U8)}
    return Spec("mu_rle_encode", order, ins, outs, ("mu_rle_encode_workspace_bytes", B, H, W, K, M),
                [("null sel", ARG, {"sel": None}), ("str_bytes off a word", ARG, {"str_bytes": lambda v: v["str_bytes"].p + 1}),
                 ("K 4097", SHAPE, {"K": 4097}), ("max_id 65537", SHAPE, {"max_id": 65537})])


def _panoptic_spec(name):
    H, W, M, _ = SHAPES[name]
    N, c = H * W, _chain(name)["pred"]
    g = lambda key, n, dt, data: Guarded(n, dt, data=data, name=key)
    ins = {"cls": g("cls", B * N, I32, c["cls"]), "ids": g("ids", B * N, I32, c["ids"]), "table": g("table", B * M * 8, I32, c["table"]),
           "score": g("score", B * M, F32, c["score"]), "count": g("count", B, I32, c["count"]), "kind": g("kind", NC, I32, [1, 1, 2]),
           "category": g("category", NC, I32, [3, 7, 11]), "B": B, "H": H, "W": W, "max_inst": M, "nc": NC, "div": 1000, "stuff": 0, "thing": 0,
           "thr": 0.0, "max_seg": M, "bgr": 0}
    order = ("cls", "ids", "table", "score", "count", "kind", "category", "B", "H", "W", "max_inst", "nc", "div", "stuff", "thing", "thr",
             "max_seg", "bgr", "seg", "seg_cls", "seg_table", "seg_score", "seg_count", "seg_order", "seg_source", "seg_values", "id_map", "rgb",
             "invalid", "ws", "ws_bytes")
    outs = {"seg": (B * N, I32), "seg_cls": (B * N, I32), "seg_table": (B * M * 8, I32), "seg_score": (B * M, F32), "seg_count": (B, I32),
            "seg_order": (B * M, I32), "seg_source": (B * M, I32), "seg_values": (B * M, I32), "id_map": (B * N, I32), "rgb": (B * N * 3, U8),
            "invalid": (B, I32)}
    return Spec("mu_panoptic", order, ins, outs, ("mu_panoptic_workspace_bytes", B, H, W, M, NC, M),
                [("null kind", ARG, {"kind": None}), ("bgr 2", ARG, {"bgr": 2}), ("num_classes 1025", SHAPE, {"nc": 1025}),
                 ("max_seg 4097", SHAPE, {"max_seg": 4097}), ("label_divisor 0", SHAPE, {"div": 0})])


def _sem_eval_spec(name):
    H, W, _, C = SHAPES[name]
    HW, Cp = H * W, (C + 31) // 32 * 32
    rng = np.random.default_rng(17)
    labels = rng.integers(0, C, size=B * HW)
    labels[::7] = 255
    ins = {"logits": Guarded(B * HW * Cp, F32, data=rng.standard_normal(B * HW * Cp).astype(np.float32), name="logits"),          # NHWC rows
           "labels": Guarded(B * HW, I64, data=labels, name="labels"), "B": B, "HW": HW, "C": C, "inner": B * HW, "outer": 0, "cs": 1, "ps": Cp,
           "ignore": 255, "inv_t": 2.0, "dtype": MU_F32}
    order = ("logits", "labels", "B", "HW", "C", "inner", "outer", "cs", "ps", "ignore", "inv_t", "img_counts", "img_loss", "confusion", "cls",
             "prob", "ws", "ws_bytes", "dtype")
    outs = {"img_counts": (B * 3 * C, I32), "img_loss": (B * 2, F64), "confusion": ((C + 1) * C, I64), "cls": (B * HW, I32), "prob": (B * HW, F32)}
    return Spec("mu_sem_eval", order, ins, outs, ("mu_sem_eval_workspace_bytes", B, HW, C),
                [("null labels", ARG, {"labels": None}), ("dtype", ARG, {"dtype": BAD}), ("C 4097", SHAPE, {"C": 4097}), ("C 0", SHAPE, {"C": 0})])


def _native_spec(name):
    h, w, _, C = SHAPES[name]
    rng = np.random.default_rng(19)
    labels, offsets, sizes = _ragged(rng, 1, C + 1)
    labels[labels == C] = 255
    n = labels.size
    ins = {"logits": Guarded(B * C * h * w, F32, data=rng.standard_normal(B * C * h * w).astype(np.float32), name="logits"),      # NCHW
           "B": B, "C": C, "h": h, "w": w, "inner": h * w, "outer": C * h * w, "cs": h * w, "ps": 1,
           "labels": Guarded(n, U8, data=labels, name="labels"), "offsets": Guarded(B + 1, I64, data=offsets, name="offsets"),
           "sizes": Guarded(B * 2, I32, data=sizes, name="sizes"), "max_h": 11, "max_w": 20, "ignore": 255, "dtype": MU_F32}
    order = ("logits", "B", "C", "h", "w", "inner", "outer", "cs", "ps", "labels", "offsets", "sizes", "max_h", "max_w", "ignore", "img_counts",
             "confusion", "valid", "classes", "ws", "ws_bytes", "dtype")
    outs = {"img_counts": (B * 3 * C, I32), "confusion": ((C + 1) * C, I64), "valid": (B, U8), "classes": (n, U8)}
    return Spec("mu_sem_eval_native", order, ins, outs, ("mu_sem_eval_native_workspace_bytes", B, C, h, w, 11, 20),
                [("null sizes", ARG, {"sizes": None}), ("dtype", ARG, {"dtype": BAD}), ("max_h 16385", ARG, {"max_h": 16385}),
                 ("C 257", SHAPE, {"C": 257}), ("h * w 65537", SHAPE, {"h": 1, "w": 65537})])


def _pil_spec(name):
    Hd, Wd, _, _ = SHAPES[name]
    C, Cp = 3, 32
    src, offsets, sizes = _ragged(np.random.default_rng(23), C, 256)
    ins = {"src": Guarded(src.size, U8, data=src, name="src"), "offsets": Guarded(B + 1, I64, data=offsets, name="offsets"),
           "sizes": Guarded(B * 2, I32, data=sizes, name="sizes"), "B": B, "C": C, "max_h": 11, "max_w": 20, "swap_rb": 1, "Hd": Hd, "Wd": Wd,
           "Cp": Cp, "dtype": MU_F32}
    order = ("src", "offsets", "sizes", "B", "C", "max_h", "max_w", "swap_rb", "dst", "u8_out", "valid", "Hd", "Wd", "Cp", "dtype", "ws", "ws_bytes")
    outs = {"dst": (B * Hd * Wd * Cp, F32), "u8_out": (B * Hd * Wd * C, U8), "valid": (B, U8)}
    # the documented convention of this entry: MU_ERR_ARG for its limits and for a short workspace
    return Spec("mu_pil_resize_u8_nhwc", order, ins, outs, ("mu_pil_resize_workspace_bytes", B, 11, 20, Hd, Wd),
                [("null offsets", ARG, {"offsets": None}), ("dtype", ARG, {"dtype": BAD}), ("C 2", ARG, {"C": 2}), ("Cp 48", ARG, {"Cp": 48}),
                 ("Hd * Wd 65537", ARG, {"Hd": 65537, "Wd": 1}), ("max_w 16385", ARG, {"max_w": 16385})], short=ARG)


SPECS = {"mu_instances": lambda name: _instances_spec(name, _chain(name)["pred"]["cls"], np.random.default_rng(3).random(B * SHAPES[name][0] * SHAPES[name][1], dtype=np.float32)),
         "mu_dbscan_instances": _dbscan_spec,
         "mu_instance_pairs": lambda name: _pairs_spec(name, _chain(name)["pred"]["ids"], _chain(name)["gt"]["ids"]),
         "mu_instance_match": _match_spec, "mu_coco_match": _coco_match_spec, "mu_id_instances": _idmap_spec, "mu_rle_encode": _rle_spec,
         "mu_panoptic": _panoptic_spec, "mu_sem_eval": _sem_eval_spec, "mu_sem_eval_native": _native_spec, "mu_pil_resize_u8_nhwc": _pil_spec}
_SPEC_CACHE = {}


def _spec(entry, name):
    if (entry, name) not in _SPEC_CACHE:
        _SPEC_CACHE[entry, name] = SPECS[entry](name)
    return _SPEC_CACHE[entry, name]


both = pytest.mark.parametrize("name", list(SHAPES))
every = pytest.mark.parametrize("entry", list(SPECS))


# ================================================================================================
# the tests
# ================================================================================================
@both
@every
def test_exact_workspace(entry, name):
    """size and carve are one statement: the queried bytes suffice (the guard band behind them stays intact), nothing past them is
    touched where there is more, and the outputs do not depend on which"""
    spec = _spec(entry, name)
    q = spec.ws_query()
    assert q > 0
    exact, _ = _run(spec, q)
    roomy, ws = _run(spec, q + EXTRA)
    for k in spec.outs:
        assert exact[k].host().tobytes() == roomy[k].host().tobytes(), (entry, k, "depends on the size of the workspace")
    assert bool((ws.t[q:] == ws.sent).all()), (entry, "wrote past the queried size of its workspace")


@both
@every
def test_short_workspace(entry, name):
    spec = _spec(entry, name)
    q = spec.ws_query()
    _refused(spec.short, spec, spec.fresh_outs(), Guarded(q, U8, name="ws"), q - 1)


@both
@every
def test_refusals(entry, name):
    """one refusal per class, each with its documented code and before anything is enqueued"""
    spec = _spec(entry, name)
    outs, ws = spec.fresh_outs(), Guarded(spec.ws_query(), U8, name="ws")
    for label, code, over in spec.refusals:
        _refused(code, spec, outs, ws, ws.n, over)
    _refused(ARG, spec, outs, ws, ws.n, {"ws": None})
