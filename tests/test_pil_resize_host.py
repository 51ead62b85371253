"""CPU: the numpy restatement of Pillow's antialiased bilinear resize (tests/_pil_reference.py) against the committed bytes of a real Pillow
(tests/golden/pil/), against the installed Pillow where there is one, and against hand-computed cases; the host side of the device path
(pack_images, the argument checks of the two entry points)."""
import os

import numpy as np
import pytest
import torch

from tests import _pil_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil")


@pytest.fixture(scope="module")
def fixtures():
    fx, version = R.load_fixtures(GOLDEN)
    assert version and len(fx) == len(list(R.fixture_cases()))
    return fx


def test_restatement_equals_every_fixture(fixtures):
    for h, w, c, kind, Hd, Wd in R.fixture_cases():
        want = fixtures[R.fixture_key(h, w, c, kind, Hd, Wd)]
        got = R.resize(R.pattern(h, w, c, kind), (Hd, Wd))
        assert got.shape == want.shape and np.array_equal(got, want), (h, w, c, kind, Hd, Wd)


def test_restatement_equals_live_pillow(fixtures):
    pytest.importorskip("PIL")
    from PIL import Image
    for h, w, c, kind, Hd, Wd in R.fixture_cases():
        src = R.pattern(h, w, c, kind)
        live = np.asarray(Image.fromarray(src).resize((Wd, Hd), Image.BILINEAR))
        assert np.array_equal(R.resize(src, (Hd, Wd)), live), (h, w, c, kind, Hd, Wd)


def test_pattern_is_the_integer_formula():
    a = R.pattern(3, 4, 3, "ramp")
    assert a.shape == (3, 4, 3) and a.dtype == np.uint8
    assert int(a[2, 3, 1]) == (3 * 3 + 2 * 5 + 40) & 255 and int(a[0, 0, 0]) == 0
    assert R.pattern(5, 7, 1, "noise").shape == (5, 7)
    b = R.pattern(64, 64, 3, "binary")
    assert set(np.unique(b)) == {0, 255} and 0.3 < (b == 255).mean() < 0.7
    n = R.pattern(64, 64, 3, "noise")
    assert len(np.unique(n)) > 200 and np.array_equal(n, R.pattern(64, 64, 3, "noise"))


def test_hand_computed_cases():
    # 1x1 -> 4x4: one tap of weight 1 everywhere
    assert np.array_equal(R.resize(np.full((1, 1), 77, np.uint8), (4, 4)), np.full((4, 4), 77, np.uint8))
    # an equal size is the identity: k = {2^22, 0}
    src = R.pattern(9, 11, 3, "noise")
    assert np.array_equal(R.resize(src, (9, 11)), src)
    xmin, n, k = R.coefficients(11, 11)
    assert np.array_equal(xmin, np.arange(11)) and np.array_equal(k[:, 0], np.full(11, 1 << 22)) and not k[:, 1:].any()
    # 2 -> 1: center 1, support 2, taps at distance .5 on either side: w = {.75, .75} / 1.5 -> k = {2^21, 2^21};
    # (2^21 + (a + b) 2^21) >> 22 = (a + b + 1) >> 1: the mean, halves rounded up
    xmin, n, k = R.coefficients(2, 1)
    assert xmin[0] == 0 and n[0] == 2 and list(k[0, :2]) == [1 << 21, 1 << 21]
    assert R.resize(np.array([[10, 13]], np.uint8), (1, 1))[0, 0] == 12
    assert R.resize(np.array([[10], [12]], np.uint8), (1, 1))[0, 0] == 11
    assert R.resize(np.array([[0, 255]], np.uint8), (1, 1))[0, 0] == 128
    assert R.resize(np.array([[255, 255]], np.uint8), (1, 1))[0, 0] == 255
    # 2x2 -> 1x1: horizontal first, its result rounded to uint8: rows {0, 1} and {1, 1} give 1 and 1, then 1 (the exact mean .75 -> 1 too);
    # {0, 1} / {0, 0}: rows give 1 and 0, then (1 + 0 + 1) >> 1 = 1, where the exact mean .25 would round to 0
    assert R.resize(np.array([[0, 1], [0, 0]], np.uint8), (1, 1))[0, 0] == 1


def test_refusal_rule():
    assert R.refused(1001, 10, 128, 128) and not R.refused(1000, 10, 128, 128) and not R.refused(400, 4, 128, 128)
    assert not R.refused(1001, 10, 1001, 5) and R.refused(0, 5, 128, 128) and R.refused(5, 0, 128, 128)
    with pytest.raises(ValueError):
        R.resize(np.zeros((1001, 10), np.uint8), (128, 128))


def test_pass_order_and_u8_intermediate_matter(fixtures):
    i = R.SIZES.index((480, 640))
    kind = R.kind_of(i)
    src, want = R.pattern(480, 640, 3, kind), fixtures[R.fixture_key(480, 640, 3, kind, 128, 128)]
    assert np.array_equal(R.resize(src, (128, 128)), want)
    vh = R.resize(src, (128, 128), order="vh")
    fl = R.resize(src, (128, 128), float_intermediate=True)
    assert 0 < (vh != want).mean() < 0.5 and int(np.abs(vh.astype(int) - want).max()) == 1
    assert 0 < (fl != want).mean() < 0.5 and int(np.abs(fl.astype(int) - want).max()) == 1


def test_to_unit_is_the_totensor_rule():
    u = np.arange(256, dtype=np.uint8)
    f = R.to_unit(u)
    assert f.dtype == np.float32 and f[0] == 0 and f[255] == 1 and np.array_equal(f, (torch.from_numpy(u).float() / 255).numpy())
    assert np.array_equal(R.to_unit(u, np.float16), (torch.from_numpy(u).float() / 255).half().numpy())


# ---- the host side of the device path ---------------------------------------------------------------------------------------------
def test_pack_images_list():
    from maskunet_amd import pack_images
    imgs = [R.pattern(5, 7, 3, "noise"), torch.from_numpy(R.pattern(1, 1, 3, "ramp")), R.pattern(4, 3, 3, "binary")]
    p = pack_images(imgs)
    assert p.data.dtype == torch.uint8 and p.offsets.dtype == torch.int64 and p.sizes.dtype == torch.int32
    assert p.offsets.tolist() == [0, 105, 108, 144] and p.sizes.tolist() == [[5, 7], [1, 1], [4, 3]]
    assert (p.channels, p.max_h, p.max_w) == (3, 5, 7) and p.data.numel() == 144
    for i, im in enumerate(imgs):
        assert np.array_equal(p.data[p.offsets[i]:p.offsets[i + 1]].numpy(), np.asarray(im).reshape(-1))
    g = pack_images([R.pattern(2, 3, 1, "noise"), R.pattern(3, 2, 1, "ramp")])
    assert g.channels == 1 and g.offsets.tolist() == [0, 6, 12] and (g.max_h, g.max_w) == (3, 3)
    g3 = pack_images([R.pattern(2, 3, 1, "noise")[:, :, None]])
    assert g3.channels == 1 and g3.sizes.tolist() == [[2, 3]]


def test_pack_images_uniform_tensor():
    from maskunet_amd import pack_images
    t = torch.from_numpy(np.stack([R.pattern(4, 6, 3, "noise"), R.pattern(4, 6, 3, "ramp")]))
    p = pack_images(t)
    assert p.offsets.tolist() == [0, 72, 144] and p.sizes.tolist() == [[4, 6], [4, 6]] and (p.max_h, p.max_w) == (4, 6)
    assert torch.equal(p.data, t.reshape(-1))


def test_pack_images_errors():
    from maskunet_amd import pack_images, resize_pil_to_nhwc
    with pytest.raises(ValueError, match="at least one"):
        pack_images([])
    with pytest.raises(ValueError, match="RGBA"):
        pack_images([np.zeros((4, 4, 4), np.uint8)])
    with pytest.raises(ValueError, match="RGBA"):
        pack_images(torch.zeros((2, 4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="share a channel count"):
        pack_images([np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError, match="uint8"):
        pack_images([np.zeros((4, 4, 3), np.float32)])
    with pytest.raises(ValueError, match=r"\[1, 16384\]"):
        pack_images([np.zeros((0, 4, 3), np.uint8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # host images and no device to send them to
        resize_pil_to_nhwc([np.zeros((4, 4, 3), np.uint8)])


def test_workspace_query_is_host_only_and_monotone():
    from maskunet_amd import _lib
    q = _lib.load().mu_pil_resize_workspace_bytes
    base = q(4, 640, 640, 128, 128)
    assert base > 0
    # room for xmin, n and ksize coefficients per output index and axis, for every image
    assert base >= 4 * 4 * 2 * 128 * (2 + 2 * 5 + 1)
    assert q(5, 640, 640, 128, 128) > base and q(4, 641, 640, 128, 128) >= base and q(4, 640, 641, 128, 128) >= base
    for a, b in ((128, 129), (129, 128), (96, 80), (3, 5)):
        assert q(1, 16384, 16384, a, b) <= q(1, 16384, 16384, a + 1, b) <= q(1, 16384, 16384, a + 1, b + 1)
    prev = 0
    for wd in range(1, 200):                                            # Wd * ceil(max_w / Wd) is not monotone; the bound is
        cur = q(1, 10, 100, 3, wd)
        assert cur >= prev
        prev = cur
    assert q(0, 640, 640, 128, 128) == -1 and q(1, 16385, 640, 128, 128) == -1 and q(1, 640, 640, 257, 256) == -1


def test_entry_point_rejects_bad_arguments_without_gpu():
    from maskunet_amd import _lib
    f = _lib.load().mu_pil_resize_u8_nhwc
    ok = dict(src=8, offsets=8, sizes=8, B=1, C=3, max_h=8, max_w=8, swap=0, dst=8, u8=None, valid=8, Hd=4, Wd=4, Cp=32, dtype=_lib.MU_F16,
              ws=8, ws_bytes=1 << 20, stream=None)
    # 8 is a non-null address that is never dereferenced: every case below fails a host check first
    for bad in (dict(src=None), dict(offsets=None), dict(sizes=None), dict(dst=None), dict(valid=None), dict(ws=None), dict(B=0), dict(C=4),
                dict(C=2), dict(C=0), dict(max_h=0), dict(max_w=16385), dict(Hd=0), dict(Hd=512, Wd=256), dict(Cp=16), dict(Cp=0), dict(dtype=2),
                dict(dtype=7), dict(ws_bytes=16)):
        args = dict(ok, **bad)
        assert f(*args.values()) == -1, bad
