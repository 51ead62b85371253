"""The row set of tools/post_host_launches.cpp: one entry point per row kind, straddling every limit and threshold of the host halves
of the seven post-processing files.  python tools/post_host_rows.py | post_host_launches"""

HW = [(1, 1), (7, 9), (8, 8), (255, 257), (256, 256), (1, 65537)]                # H*W = 1, odd, 64, 65535, 65536, 65537
INST = [1, 5, 8, 4096, 4097]                                                    # max_inst: 1, not a power of two, the limit +- 1
rows = []


def row(kind, *values):
    rows.append(" ".join([kind] + [str(v) for v in values]))


for B in (1, 2):
    for H, W in HW:
        for m in INST:
            row("instances", B, H, W, m)
            row("pairs", B, H, W, m, 5)
            row("pairs", B, H, W, 5, m)
for H, W in HW:
    for D in (1, 4, 5, 16, 17, 32, 33, 64, 65):
        row("dbscan", 2, H, W, D, 3, 5, 2, 500)
for nc in (1, 3, 1023, 1024, 1025):
    for m in INST:
        row("dbscan", 2, 7, 9, 5, nc, m, 2, 500)
for B in (1, 65535, 65536):
    row("dbscan", B, 8, 8, 5, 3, 8, 1, 250)
for nc in (1, 3, 1023, 1024, 1025):
    for T in (1, 2, 32, 33):
        for mp, K in ((5, 4), (5, 5), (5, 6), (8, 8), (4096, 4096), (4096, 4097), (4097, 4097)):
            row("match", 2, 7, 9, mp, 5, nc, K, 100, T)
            for A in (0, 1, 2, 4, 5):
                row("coco_match", 2, 7, 9, mp, 8, nc, K, 100, T, A)
for H, W in HW:
    row("match", 2, H, W, 8, 4096, 3, 5, 1, 2)
    row("coco_match", 2, H, W, 8, 4097, 3, 5, 1, 2, 2)
    for m in INST:
        for cap in (1, 4, 1023, 1024, 1025):
            row("idmap", 2, H, W, m, cap)
    for K in (1, 5, 4096, 4097):
        for max_id in (1, 5, 65536, 65537):
            for mis in (0, 1, 3):
                row("rle", 2, H, W, K, max_id, mis)
        for L in (0, 1, 2 * H * W + K, 2**31 - 1, 2**31):
            row("rle_decode", 2, H, W, K, L)
for B, Ho, Wo in ((2, 7, 9), (2, 256, 256), (2, 1, 65537), (15, 256, 256), (16, 255, 257), (16, 256, 256), (17, 256, 256)):
    for A in (0, 2):
        for n_points, n_counts in ((0, 0), (40, 0), (0, 40), (0x3FFFFFFF, 0x7FFFFFFF), (0x40000000, 5), (5, 0x80000000)):
            for max_points in (1, 1 << 21, (1 << 21) + 1):
                row("coco_masks", B, A, 3, n_points, n_counts, Ho, Wo, max_points)
for H, W in HW:
    for m, s in ((5, 5), (8, 5), (5, 8), (4096, 4096), (4097, 5), (5, 4097)):
        for nc in (1, 3, 1023, 1024, 1025):
            row("panoptic", 2, H, W, m, nc, s, 1000, 64, 0, 0)
for div, sl, tl, bgr in ((0, 0, 0, 0), (1, -1, 0, 1), (1, 0, -1, 1), (1000, 4096, 4096, 1)):
    row("panoptic", 2, 8, 8, 5, 3, 5, div, sl, tl, bgr)
# mu_sem_eval: the vector-width steps of both dtypes, the LDS confusion limit, the 48 KiB grant threshold (C = 108 / 109), both layouts
SEM_C = (1, 5, 40, 63, 64, 65, 108, 109, 128, 129, 150, 192, 193, 256, 257, 384, 385, 4096, 4097)
for B, hw in ((1, 1), (2, 63), (2, 64), (1, 511), (1, 512), (1, 513), (64, 16384), (512, 16384), (513, 16384), (1, 2**31 - 1), (1, 2**31)):
    for C in SEM_C:
        Cp = (C + 31) // 32 * 32
        for prob in (0, 1):
            row("sem_eval", B, hw, C, B * hw, 0, 1, Cp, 0, prob)                 # NHWC rows, padded channels
        row("sem_eval", B, hw, C, hw, C * hw, hw, 1, 0, 1)                       # NCHW: strided
for C in (5, 64, 109, 193):
    Cp = (C + 31) // 32 * 32
    row("sem_eval", 2, 64, C, 128, 0, 1, Cp, 4, 0)                               # logits off a 16-byte boundary
    row("sem_eval", 2, 64, C, 128, 0, 1, Cp + 2, 0, 0)                           # a row stride the vectors do not divide
    row("sem_eval", 2, 64, C, 64, 64 * Cp + 2, 1, Cp, 0, 0)                      # an outer stride they do not divide
    row("sem_eval", 2, 64, C, 128, 0, 2, 2 * Cp, 0, 0)                           # c_stride != 1
    row("sem_eval", 2, 64, C, 128, 0, 1, C, 0, 0)                                # rows shorter than their vectors (where C % VN)
    row("sem_eval", 2, 64, C, 0, 0, 1, Cp, 0, 0)                                 # inner < 1
for C in (1, 5, 19, 40, 150, 255, 256, 257):
    for h, w in ((1, 1), (7, 9), (8, 8), (32, 32), (255, 257), (256, 256), (1, 65537)):
        row("native", 2, C, h, w, 37, 53)
for B, mh, mw in ((2, 1, 1), (2, 16, 64), (2, 17, 65), (2, 16384, 16384), (2, 16385, 64), (2, 64, 16385), (8191, 16384, 16384), (8192, 16384, 16384)):
    row("native", B, 19, 8, 8, mh, mw)
for C in (1, 2, 3, 4):
    for Cp in (0, 32, 48, 64):
        row("pil", 2, C, 37, 53, 7, 9, Cp)
for B, mh, mw, Hd, Wd in ((2, 37, 53, 256, 256), (2, 37, 53, 255, 257), (2, 37, 53, 1, 65537), (2, 16384, 16384, 8, 8), (2, 16385, 64, 8, 8),
                          (2, 64, 16385, 8, 8), (255, 64, 64, 1, 65535), (256, 64, 64, 1, 65535), (257, 64, 64, 1, 65535), (2, 64, 64, 0, 8)):
    for C in (1, 3):
        row("pil", B, C, mh, mw, Hd, Wd, 32)
print("\n".join(rows))
