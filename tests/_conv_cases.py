"""One table of convolution shapes for the kernel suite.

CONV_CASES / H2_SHAPES are the real-valued parity cases of tests/_gpu_checks.check_conv and of
test_conv3x3_two_term_backward_through_the_abi.  LAYERS is the table of the plan-coverage test (CPU) and of the bit-exact integer
tests (GPU): every plan id of every mu_conv_*_plan query is reached by at least one of its rows, and both sides of every numeric
threshold of the selection functions are rows of it (EDGES)."""

# (B, H, W, Cin, Cout, k): valid (unpadded) channel counts, through maskunet_amd.ops
CONV_CASES = [(2, 12, 12, 32, 32, 3), (1, 16, 16, 64, 128, 3), (2, 8, 8, 128, 64, 3), (1, 10, 6, 19, 32, 3),
              (1, 8, 8, 64, 150, 1), (2, 9, 7, 256, 256, 3), (1, 16, 16, 3, 64, 3), (2, 8, 8, 32, 1, 1),
              (1, 6, 6, 512, 256, 3),
              # W % 32 == 0: the 3-taps-per-block / 9-taps-per-block weight-gradient kernels (fp16) incl. row/image borders
              (2, 32, 32, 64, 64, 3), (1, 64, 32, 128, 128, 3), (2, 16, 64, 64, 128, 3), (1, 32, 32, 256, 128, 3),
              # 16x16-tile ping-pong kernel: odd number of 64-channel chunks, non-square image, two channel blocks
              (2, 32, 48, 192, 256, 3), (3, 16, 16, 128, 128, 3),
              # first-layer weight-gradient kernel (<= 3 valid input channels): ragged width, two channel blocks, 1 channel
              (2, 20, 24, 3, 128, 3), (1, 8, 8, 1, 64, 3),
              # its matrix-core form (fp16, W % 32 == 0): one row per block, two channel blocks, 2 valid channels, bands of two rows
              # that straddle image borders (4 x 255 rows over 512 blocks), four k-steps per row
              (2, 8, 32, 3, 64, 3), (1, 5, 64, 3, 128, 3), (3, 4, 96, 2, 64, 3), (4, 255, 32, 3, 64, 3), (1, 6, 128, 3, 64, 3),
              # nine-taps-per-block weight-gradient kernel (fp16, 64-channel-wide layers, W % 32 == 0, W <= 128): bands of two rows
              # that straddle image borders, W = 96 / 128, both mixed channel shapes
              (4, 99, 32, 64, 64, 3), (2, 5, 96, 64, 64, 3), (1, 6, 128, 128, 64, 3), (2, 7, 64, 64, 128, 3),
              # its 16-pixel-wide form (a k-step = a pair of image rows): bands of four rows over images of six rows, 128 -> 256
              (100, 6, 16, 64, 64, 3), (3, 4, 16, 128, 256, 3),
              # weights-resident kernel in its two-halves form (fp16, 64 -> 128 without a statistics epilogue, >= 1024 tiles)
              (16, 128, 128, 64, 128, 3),
              # 16-pixel-wide images, 128-wide layers
              (2, 8, 16, 256, 128, 3), (5, 16, 16, 64, 64, 3),
              # shapes around the kernel-selection edges: 80-wide (16x16 conv tiles, one-tap weight-grad), 192-wide (64-pixel
              # weight-grad stages), 32-wide with even / odd height (two-row stages / flat stages), persistent conv with a tail
              (2, 48, 80, 64, 128, 3), (1, 32, 192, 128, 128, 3), (2, 6, 32, 128, 128, 3), (1, 5, 32, 128, 128, 3),
              (5, 64, 64, 64, 128, 3),
              # weights-resident persistent kernel (fp16, 64 -> 64, >= 512 tiles of 16 x 16 pixels): two to three tiles per block
              # (each of its two wave groups one or two), ragged tail, non-square images
              (10, 128, 112, 64, 64, 3), (3, 192, 240, 64, 64, 3),
              # 1x1 layers: q/k/v projection shapes (Cout = 3C: row-staged epilogue, single-stage Cin = 64 kernel, wide
              # weight-grad tiles), their data-gradient shape, the 150-class head with a ragged pixel count
              (2, 9, 7, 64, 192, 1), (1, 16, 16, 128, 384, 1), (2, 5, 5, 256, 768, 1), (3, 7, 9, 192, 64, 1), (2, 33, 17, 64, 150, 1),
              (1, 40, 40, 64, 192, 1)]

# (B, H, W, Cin, Cout): the ping-pong kernel (Cin of the layer % 128, H % 16), the halo-tile kernel at 128 / 64 output channels, the
# generic register-staged kernel (odd sizes, 32-channel operands)
H2_SHAPES = [(2, 32, 32, 128, 128), (1, 16, 16, 256, 64), (2, 8, 16, 64, 128), (1, 24, 16, 64, 64), (2, 13, 9, 32, 64), (1, 7, 20, 96, 32),
             (1, 16, 16, 512, 512), (1, 8, 16, 128, 64), (1, 24, 32, 256, 128)]      # (the last two: the 128-channel halo-tile form, H % 16 != 0)


def pad32(c):
    return (c + 31) // 32 * 32


def L(B, H, W, cin, cout, taps=9, heavy=False):
    """A layer: valid channel counts cin -> cout (zero-padded to multiples of 32, as the model stores them)."""
    return dict(B=B, H=H, W=W, cin=cin, cout=cout, Cin=pad32(cin), Cout=pad32(cout), taps=taps, heavy=heavy)


def name_of(c):
    return f"{c['B']}x{c['H']}x{c['W']}_{c['cin']}to{c['cout']}_k{3 if c['taps'] == 9 else 1}"


# Both sides of each numeric threshold of a *_pick function: (what, query, dtype, row just below, row at).  query: "fwd_stats" =
# mu_conv_fwd_plan(with_stats = 1), "fwd" = with_stats = 0, "wgrad" = mu_conv_wgrad_plan(pair = 0).  Rows marked heavy run the entries
# the threshold concerns only (their CPU references are the expensive ones).
EDGES = [
    ("MU_NT5_MINTILES = 512 tiles of 16 x 16", "fwd_stats", "fp16", L(7, 16, 1168, 64, 64), L(8, 16, 1024, 64, 64)),
    ("MU_NT5_SPLIT_MINTILES = 1024 tiles", "fwd", "fp16", L(3, 176, 496, 64, 128, heavy=True), L(4, 256, 256, 64, 128, heavy=True)),
    ("persistent nt4p: t16 * (Cout / 128) >= 1024", "fwd_stats", "fp16", L(3, 80, 272, 64, 512, heavy=True), L(4, 128, 128, 64, 512, heavy=True)),
    ("persistent nt4p: Cin <= 256", "fwd_stats", "fp16", L(4, 128, 128, 256, 512, heavy=True), L(4, 128, 128, 320, 512, heavy=True)),
    ("nt4x: t16 * (Cout / 128) >= 192", "fwd_stats", "fp32x", L(1, 16, 3056, 64, 128), L(3, 128, 128, 64, 128, heavy=True)),
    ("weight ring: Cin * element size >= 256 (fp16)", "fwd_stats", "fp16", L(2, 8, 16, 64, 64), L(2, 8, 16, 128, 64)),
    ("weight ring: Cin * element size >= 256 (fp32)", "fwd", "fp32", L(2, 8, 16, 32, 64), L(2, 8, 16, 64, 64)),
    ("first-layer kernels: cin_valid <= 3", "wgrad", "fp16", L(2, 8, 32, 3, 64), L(2, 8, 32, 4, 64)),
    ("first-layer kernels: W <= MU_RGB_MAXW = 256", "wgrad", "fp16", L(1, 4, 256, 3, 64), L(1, 4, 288, 3, 64)),
    ("wgrad9: W <= 128", "wgrad", "fp16", L(1, 6, 128, 64, 64), L(1, 6, 160, 64, 64)),
    ("wgrad9: channels <= MU_WG9_MAXC32 = 128 at W = 32", "wgrad", "fp16", L(2, 6, 32, 128, 128), L(2, 6, 32, 192, 128)),
    ("wgrad9_w16: channels <= MU_WG9_MAXC16 = 512", "wgrad", "fp16", L(2, 8, 16, 512, 64), L(2, 8, 16, 576, 64)),
]

LAYERS = [
    # ---- 3x3 forward / fused / data gradient: every halo-tile kernel and the kernels behind them
    L(2, 12, 12, 32, 32),                   # generic 32-wide tile (W % 16 != 0)
    L(2, 9, 7, 64, 64), L(2, 9, 7, 256, 128),      # generic 64 / 128 tiles
    L(2, 12, 16, 64, 64), L(1, 12, 16, 64, 128),   # H % 8 != 0: LDS-DMA 64 / 128 forms
    L(1, 24, 16, 64, 64), L(1, 24, 32, 256, 128), L(1, 8, 16, 128, 64),     # H % 16 == 8: halo tiles of 8 rows
    L(2, 32, 48, 192, 256), L(3, 16, 16, 128, 128),                         # ping-pong: odd number of 64-channel chunks
    L(1, 16, 16, 512, 512),                                                 # K = 4608
    L(2, 32, 32, 256, 256),
    L(10, 128, 112, 64, 64, heavy=True), L(3, 192, 240, 64, 64, heavy=True),      # weights-resident: two / three tiles per block, ragged tail
    L(5, 64, 64, 64, 128), L(2, 48, 80, 64, 128),
    L(2, 144, 304, 64, 384, heavy=True),    # >= 1024 block-tiles but three channel blocks: not persistent
    # ---- first layer (padded 3 / 2 / 1 -> 64 / 128): plain-FMA and matrix-core weight gradients, bands that straddle image borders
    L(2, 20, 24, 3, 128), L(1, 8, 8, 1, 64), L(2, 8, 32, 3, 64), L(1, 5, 64, 3, 128), L(3, 4, 96, 2, 64), L(4, 255, 32, 3, 64),
    L(1, 6, 128, 3, 64), L(1, 3, 160, 3, 64), L(1, 3, 192, 1, 64), L(1, 3, 224, 3, 64), L(1, 16, 16, 3, 64),
    # ---- padded class counts: 19 / 133 / 150 valid channels inside 32-multiples
    L(1, 10, 6, 19, 32), L(2, 16, 16, 19, 64), L(1, 16, 16, 133, 64), L(2, 8, 16, 64, 133),
    # ---- weight gradient families
    L(4, 99, 32, 64, 64), L(2, 5, 96, 64, 64), L(1, 6, 128, 128, 64), L(2, 7, 64, 64, 128),         # wgrad9: 1..4 k-steps per row
    L(100, 6, 16, 64, 64), L(3, 4, 16, 128, 256),                                                   # wgrad9_w16
    L(2, 8, 16, 1024, 128), L(1, 32, 32, 256, 128), L(1, 32, 192, 128, 128), L(1, 5, 96, 128, 128),  # wgrad3 128 x 128: w16 / rows2 / flat64 / plain
    L(2, 8, 16, 1024, 64), L(1, 32, 32, 256, 64), L(1, 8, 64, 192, 128), L(1, 5, 96, 192, 128),      # wgrad3 64 x 64: the same four
    L(1, 5, 32, 256, 256),                                                                           # odd height at W = 32: flat stages
    # ---- 1x1 layers: q/k/v projections, their data gradient, the class heads, generic tiles
    L(2, 9, 7, 64, 192, 1), L(1, 16, 16, 128, 384, 1), L(2, 5, 5, 256, 768, 1), L(3, 7, 9, 192, 64, 1), L(1, 40, 40, 64, 192, 1),
    L(2, 33, 17, 64, 150, 1), L(2, 16, 16, 128, 150, 1), L(1, 16, 24, 64, 133, 1), L(2, 8, 8, 32, 1, 1), L(2, 8, 8, 64, 19, 1),
    L(1, 8, 8, 96, 64, 1), L(1, 8, 8, 96, 128, 1), L(1, 16, 16, 128, 128, 1), L(1, 16, 16, 64, 64, 1), L(2, 8, 8, 192, 192, 1),
]
for _e in EDGES:
    for _c in _e[3:]:
        if _c not in LAYERS:
            LAYERS.append(_c)


# ------------------------------------------------------------------------------------------------
# which kernel each entry point runs for a row (host-only queries of the built library)
# ------------------------------------------------------------------------------------------------
DTYPES = {"fp32": 0, "fp16": 1, "fp32x": 2}
OPS = {"fwd": 0, "fused": 1, "dgrad_h": 2, "wgrad": 3}


def plan_name(op, pid):
    from maskunet_amd import _lib
    s = _lib.load().mu_conv_plan_name(OPS[op], pid)
    return s.decode() if s else None


def all_plan_names(op):
    from maskunet_amd import _lib
    lib = _lib.load()
    names = [plan_name(op, i) for i in range(1, lib.mu_conv_plan_count(OPS[op]))]
    return [n for n in names if n is not None]


def entries(c):
    """[(entry, dtype name, op, plan id)] for every entry point / dtype the exact tests run on the row c."""
    from maskunet_amd import _lib
    lib = _lib.load()
    B, H, W, Cin, Cout, taps, cin = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["taps"], c["cin"]
    out = []
    for dn, d in DTYPES.items():
        out.append(("fwd", dn, "fwd", lib.mu_conv_fwd_plan(B, H, W, Cin, Cout, taps, d, 0)))
        if lib.mu_conv_stats_rows(B, H, W, Cin, Cout, taps, d) > 0:
            out.append(("fwd_stats", dn, "fwd", lib.mu_conv_fwd_plan(B, H, W, Cin, Cout, taps, d, 1)))
        out.append(("fused", dn, "fused", lib.mu_conv_fwd_fused_plan(B, H, W, Cin, Cout, taps, d)))
        if dn == "fp32x" and taps == 9 and cin > 3:
            out.append(("dgrad_h", dn, "dgrad_h", lib.mu_conv_dgrad_h_plan(B, H, W, Cout, Cin)))
            out.append(("wgrad_h", dn, "wgrad", lib.mu_conv_wgrad_plan(B, H, W, Cin, Cout, 9, cin, DTYPES["fp16"], 1)))
            out.append(("wgrad_h1", dn, "wgrad", lib.mu_conv_wgrad_plan(B, H, W, Cin, Cout, 9, cin, DTYPES["fp16"], 0)))
        elif not (dn == "fp32x" and taps == 9):          # (fp32x hands its <= 3-channel first layer to mu_conv_wgrad as plain fp32)
            out.append(("wgrad", dn, "wgrad", lib.mu_conv_wgrad_plan(B, H, W, Cin, Cout, taps, cin, d, 0)))
        if dn == "fp16":
            # the fp16 data gradient: mu_conv_fwd on mode-1 weights, no statistics (Cout -> Cin)
            out.append(("dgrad", dn, "fwd", lib.mu_conv_fwd_plan(B, H, W, Cout, Cin, taps, d, 0)))
            if lib.mu_conv_wgrad_bias_supported(Cin, Cout, taps, d):
                out.append(("wgrad_bias", dn, "wgrad", lib.mu_conv_wgrad_bias_plan(B, H, W, Cin, Cout, taps, cin, d)))
    if c["heavy"]:          # large rows exist for the forward selection: forward entries only (one CPU reference, shared by the dtypes)
        out = [e for e in out if e[0] in ("fwd", "fwd_stats")]
    return out


def model_layers(c_out, three_head, hw=128):
    """[(parameter name, Cin, Cout, taps, cin_valid, H)] of every convolution of UNet(3, c_out) / InstanceUNet(3, c_out, 16) at hw x hw,
    from the oracle's state layout: the 3x3 / 1x1 conv weights, and the q/k/v projections of each attention block as the one
    [3C, C] 1x1 layer the HIP path runs."""
    from oracle import maskunet_oracle as O
    res = {"initial_conv": 1, "downsample1": 2, "self_attention1": 2, "downsample2": 4, "self_attention2": 4, "downsample3": 8,
           "self_attention3": 8, "bottom1": 8, "bottom2": 8, "bottom3": 8, "upsample1": 4, "self_attention4": 4, "upsample2": 2,
           "self_attention5": 2, "upsample3": 1, "self_attention6": 1, "final_layer": 1, "boundary_head": 1, "embedding_head": 1}
    out = []
    for key, shape, _ in O.unet_state_shapes(3, c_out, three_head, 16, hw):
        top = key.split(".")[0]
        if len(shape) == 4:
            out.append((key, pad32(shape[1]), pad32(shape[0]), shape[2] * shape[3], shape[1], hw // res[top]))
        elif key.endswith(".query.weight"):
            out.append((top + ".qkv", pad32(shape[1]), 3 * shape[0], 1, shape[1], hw // res[top]))
    return out
