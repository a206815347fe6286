"""float64 reference of the encoder's layers, one at a time, for tests/test_gpu_encoder_layers.py and its interpreter mirror
tests/test_encoder_layers_sim.py.  Torch float64 only (on whatever device the tensors live); never calls the library.

Every function takes the values the kernel actually READ -- the stored bf16 (or f32) tensor of the layer below, the f32 master weights
rounded to the compute dtype -- and returns the exact result together with S, the float64 sum of the absolute values of the terms of
each element.  An element is held to

    bf16-stored output:   |got - ref| <= 2^-8 |ref| + 2^-14 S      (one bf16 rounding of the output + f32 accumulation)
    f32 output:           |got - ref| <= 2^-14 S                   (f32 parity mode: 2^-20 S for every output)

All tensors are NHWC; 3x3 weights are HWIO [3, 3, Cin, Cout] as the parameters store them."""
import torch
import torch.nn.functional as F

REL_BF16 = 2.0 ** -8
ABS_BF16 = 2.0 ** -14
ABS_F32 = 2.0 ** -20


def bf16_round(t):
    """float -> the nearest bf16 (ties to even), as float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


# ------------------------------------------------------------------------------------------------------------------ convolutions --
def conv1_pre(img_u8, w, b, round_w):
    """encoder.py:26-32 without the ReLU: u8 image [B, H, W] -> (x - 128) / 128 -> 3x3 SAME conv 1 -> 64 + bias.  round_w: the bf16
    mode's MFMA kernels read the weights rounded to bf16 (c1_wop); the image values are exact in bf16."""
    x = (img_u8.to(torch.float64) - 128.0) / 128.0
    w = w.to(torch.float64)
    if round_w:
        w = bf16_round(w)
    return conv3x3(x[..., None], w, b, 1)


def conv3x3(x, w, b, pad, addend=None):
    """y[b, o] = sum_k x[b, o + k - pad] w[k] (+ bias) (+ addend [Ho*Wo, Cout], broadcast over the batch): pad 1 = SAME, 0 = VALID.
    -> (y before any activation, S = |x| * |w| + |b| + |addend|)."""
    x = x.to(torch.float64)
    w = w.to(torch.float64)
    Bn, H, W, _ = x.shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    ax, aw = xp.abs(), w.abs()
    y = torch.zeros(Bn, Ho, Wo, w.shape[3], dtype=torch.float64, device=x.device)
    s = torch.zeros_like(y)
    for kh in range(3):
        for kw in range(3):
            y += xp[:, kh:kh + Ho, kw:kw + Wo] @ w[kh, kw]
            s += ax[:, kh:kh + Ho, kw:kw + Wo] @ aw[kh, kw]
    if b is not None:
        b = b.to(torch.float64)
        y += b
        s += b.abs()
    if addend is not None:
        a = addend.to(torch.float64).reshape(Ho, Wo, -1)
        y += a
        s += a.abs()
    return y, s


def conv3x3_dgrad(dy, w, pad):
    """data gradient of conv3x3(., w, pad): dx[b, i] = sum_k dy[b, i - k + pad] w[k]^T (pad 0 = the VALID conv's, a pad-2 correlation
    with the flipped kernel).  -> (dx, S)."""
    dy = dy.to(torch.float64)
    w = w.to(torch.float64)
    Bn, Ho, Wo, _ = dy.shape
    Hi, Wi = Ho + 2 - 2 * pad, Wo + 2 - 2 * pad
    dp = F.pad(dy, (0, 0, 2, 2, 2, 2))
    ad, aw = dp.abs(), w.abs()
    dx = torch.zeros(Bn, Hi, Wi, w.shape[2], dtype=torch.float64, device=dy.device)
    s = torch.zeros_like(dx)
    for kh in range(3):
        for kw in range(3):
            y0, x0 = pad + 2 - kh, pad + 2 - kw
            dx += dp[:, y0:y0 + Hi, x0:x0 + Wi] @ w[kh, kw].T
            s += ad[:, y0:y0 + Hi, x0:x0 + Wi] @ aw[kh, kw].T
    return dx, s


def conv3x3_wgrad(x, dy, pad):
    """dW[kh, kw] = sum over pixels of x[b, o + k - pad] (outer) dy[b, o].  -> (dW [3, 3, Cin, Cout], S = sum |x dy|)."""
    x = x.to(torch.float64)
    dy = dy.to(torch.float64)
    Ho, Wo, Co = dy.shape[1], dy.shape[2], dy.shape[3]
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    d2 = dy.reshape(-1, Co)
    ad = d2.abs()
    Ci = x.shape[3]
    dw = torch.zeros(3, 3, Ci, Co, dtype=torch.float64, device=x.device)
    s = torch.zeros_like(dw)
    for kh in range(3):
        for kw in range(3):
            sl = xp[:, kh:kh + Ho, kw:kw + Wo].reshape(-1, Ci)
            dw[kh, kw] = sl.T @ d2
            s[kh, kw] = sl.abs().T @ ad
    return dw, s


def colsum(d):
    """bias gradient: column sums over every pixel.  -> (sum, S = sum |d|)."""
    d = d.to(torch.float64).reshape(-1, d.shape[-1])
    return d.sum(0), d.abs().sum(0)


def relu_mask(d, y):
    """ReLU-masked data gradient: d where the stored activation y is > 0, else 0."""
    return torch.where(y > 0, d.to(torch.float64), torch.zeros((), dtype=torch.float64, device=d.device))


# ------------------------------------------------------------------------------------------- the "cnn" variant's strided conv --
def im2col_s2(y):
    """(2, 4) stride-2 TF SAME patches (rows pad 0 above, columns 1 to the left): cols[(b, oy, ox)][(kh * 4 + kw) * C + c] =
    y[b, 2 oy + kh, 2 ox + kw - 1, c], zero outside.  -> [B, Ho, Wo, 8 C]."""
    Bn, H, W, C = y.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    yp = F.pad(y, (0, 0, 1, 2 * Wo + 2 - W, 0, 2 * Ho - H))
    taps = [yp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(2) for kw in range(4)]
    return torch.cat(taps, dim=3)


def strided_conv(cols, w, b):
    """p = cols @ W + b, no activation; w [2, 4, C, C] (HWIO) -> [8C, C].  -> (p, S)."""
    wm = w.to(torch.float64).reshape(-1, w.shape[3])
    c = cols.to(torch.float64)
    b = b.to(torch.float64)
    return c @ wm + b, c.abs() @ wm.abs() + b.abs()


def strided_conv_bwd(cols, dp, w):
    """backward of strided_conv on its stored operands: (db, S), (dW [2, 4, C, C], S), (d_cols = dp W^T [B, Ho, Wo, 8 C], S)."""
    Bn, Ho, Wo, C = dp.shape
    d2 = dp.to(torch.float64).reshape(-1, C)
    c2 = cols.to(torch.float64).reshape(-1, cols.shape[3])
    wm = w.to(torch.float64).reshape(-1, C)
    db, sdb = d2.sum(0), d2.abs().sum(0)
    dw, sdw = (c2.T @ d2).reshape(w.shape), (c2.abs().T @ d2.abs()).reshape(w.shape)
    dcol, scol = d2 @ wm.T, d2.abs() @ wm.abs().T
    return (db, sdb), (dw, sdw), (dcol.reshape(Bn, Ho, Wo, 8 * C), scol.reshape(Bn, Ho, Wo, 8 * C))


def col2im_s2_relu(dcols, y):
    """the transpose of im2col_s2 on stored d_cols (each pixel sums the <= 2 windows that cover it), masked by the stored y > 0.
    -> (d_y [B, H, W, C], S)."""
    Bn, Ho, Wo, C8 = dcols.shape
    C = C8 // 8
    H, W = y.shape[1], y.shape[2]
    t = dcols.to(torch.float64).reshape(Bn, Ho, Wo, 8, C)

    def fold(t):
        out = torch.zeros(Bn, 2 * Ho, 2 * Wo + 2, C, dtype=torch.float64, device=t.device)    # column 0 = x = -1
        for kh in range(2):
            for kw in range(4):
                out[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo - 1:2] += t[:, :, :, kh * 4 + kw]
        return out[:, :H, 1:W + 1]
    return relu_mask(fold(t), y), relu_mask(fold(t.abs()), y)


# ------------------------------------------------------------------------------------------------------------------------ pools --
def windows(v, ph, pw, fill):
    """SAME pool windows (window == stride), clipped at the bottom / right edge: [B, H, W, C] -> [B, Hq, Wq, C, ph * pw] in scan order
    (qy * pw + qx), positions outside the image = fill; and valid [Hq, Wq, ph * pw]."""
    Bn, H, W, C = v.shape
    Hq, Wq = -(-H // ph), -(-W // pw)
    vp = F.pad(v, (0, 0, 0, Wq * pw - W, 0, Hq * ph - H), value=fill)
    out = vp.reshape(Bn, Hq, ph, Wq, pw, C).permute(0, 1, 3, 5, 2, 4).reshape(Bn, Hq, Wq, C, ph * pw)
    ok = torch.zeros(Hq * ph, Wq * pw, dtype=torch.bool, device=v.device)
    ok[:H, :W] = True
    return out, ok.reshape(Hq, ph, Wq, pw).permute(0, 2, 1, 3).reshape(Hq, Wq, ph * pw)


def pool_ref(pre, S, ph, pw, rel=REL_BF16, absf=ABS_BF16):
    """ReLU + SAME max-pool of the pre-activation `pre` (float64) whose elements carry the sums S.  Per pooled element -> dict:
      value  max over the clipped window of relu(pre)            bound  max over the window of rel |value| + absf S
      first  the first maximum's position in scan order          cand   positions whose bound overlaps the maximum's (bool [.., ph*pw])
      exact  True where every candidate equals the maximum exactly in float64 (a clear tie: the FIRST position must win) -- a tie at 0
             counts only if every candidate's pre-activation is below -bound (else the kernel may see a tiny positive value there)
      pos    the pre-activation maximum (bit 4 = it is > 0) and `pre_max`."""
    neg = -float("inf")
    v, ok = windows(torch.relu(pre), ph, pw, neg)
    p, _ = windows(pre, ph, pw, neg)
    s, _ = windows(S, ph, pw, 0.0)
    vmax, first = v.max(dim=-1)
    okb = ok[:, :, None, :]
    zero = torch.zeros((), dtype=v.dtype, device=v.device)
    bq = torch.where(okb, rel * v.abs() + absf * s, zero)                     # each position's own bound
    bound = bq.amax(-1)
    # the kernel compares its own (rounded) values: a position may beat the maximum where the two bounds overlap
    bfirst = torch.gather(bq, -1, first[..., None])
    cand = okb & (v + bq >= vmax[..., None] - bfirst)
    true = torch.ones((), dtype=torch.bool, device=v.device)
    exact_vals = torch.where(cand, v == vmax[..., None], true).all(-1)
    clear_zero = torch.where(cand, p < -bq, true).all(-1)
    exact = exact_vals & ((vmax > 0) | clear_zero)
    return dict(value=vmax, first=first, bound=bound, cand=cand, exact=exact, pre_max=p.max(-1)[0], valid=ok)


def route(dp, mask, ph, pw, H, W):
    """pool backward from a mask byte per pooled element (position | 4 if the maximum was positive): d_y at the mask's position where bit
    4 is set, else 0.  Works on the raw bit patterns (int16 / int32 views) so that it can be compared bit for bit.  -> [B, H, W, C]."""
    Bn, Hq, Wq, C = dp.shape
    m = mask.to(torch.int64)
    pos, on = m & 3, (m & 4) != 0
    z = torch.zeros((), dtype=dp.dtype, device=dp.device)
    g = torch.where(on, dp, z)
    out = torch.stack([torch.where(pos == q, g, z) for q in range(ph * pw)], dim=-1)      # [B, Hq, Wq, C, ph * pw]
    out = out.reshape(Bn, Hq, Wq, C, ph, pw).permute(0, 1, 4, 2, 5, 3).reshape(Bn, Hq * ph, Wq * pw, C)
    return out[:, :H, :W].contiguous()


def route_by_first_max(dp, y, ph, pw):
    """the unfused pool backward of the f32 parity mode (maxpool_relu_bwd): d_p routed to the first maximum of the STORED activation y
    in scan order, nothing where that maximum is not positive.  Exact on the stored operands.  -> d_y [B, H, W, C] float64."""
    Bn, H, W, C = y.shape
    v, ok = windows(y.to(torch.float64), ph, pw, -float("inf"))
    vmax, first = v.max(dim=-1)
    g = torch.where(vmax > 0, dp.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dp.device))
    out = torch.stack([torch.where(first == q, g, torch.zeros_like(g)) for q in range(ph * pw)], dim=-1)
    out = out.reshape(Bn, v.shape[1], v.shape[2], C, ph, pw).permute(0, 1, 4, 2, 5, 3).reshape(Bn, v.shape[1] * ph, v.shape[2] * pw, C)
    return out[:, :H, :W].contiguous()


def conv1_pool_bwd(img_u8, w, b, dp1, round_w, absf=ABS_BF16):
    """layer 1's backward (conv1 recomputed in f32 from exact operands, the gradient of the pooled ReLU output routed to the first maximum
    of each window, dW1 and db1) on the stored d_p1.  The kernel decides on unrounded f32 sums, so only a window whose candidates lie within
    absf S of each other (and are not an exact tie) may be routed to another of them, and only one whose maximum + bias lies within absf S of
    0 may pass or drop its gradient: their possible share of dW1 / db1 is returned as an extra allowance.
    -> (dW1 [3, 3, 1, 64], S, allowance), (db1, S, allowance)."""
    pre, S = conv1_pre(img_u8, w, b, round_w)
    Bn, H, W, _ = pre.shape
    pr = pool_ref(pre, S, 2, 2, 0.0, absf)
    x = (img_u8.to(torch.float64) - 128.0) / 128.0
    xp = F.pad(x, (1, 1, 1, 1))
    # patch of every full-resolution pixel: [B, H, W, 9]
    patch = torch.stack([xp[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)], dim=-1)
    pw_, _ = windows(patch, 2, 2, 0.0)                                           # [B, Hq, Wq, 9, 4]
    d = dp1.to(torch.float64)
    zero = torch.zeros_like(d)
    gref = torch.where(pr["pre_max"] > 0, d, zero)
    amb_relu = pr["pre_max"].abs() <= pr["bound"]
    sel = F.one_hot(pr["first"], 4).to(torch.float64)                           # [B, Hq, Wq, 64, 4]
    # dW[t, c] = sum over windows of patch[t, first] * gref[c]
    xf = torch.einsum("bhwtq,bhwcq->bhwtc", pw_, sel)
    dw = torch.einsum("bhwtc,bhwc->tc", xf, gref)
    sdw = torch.einsum("bhwtc,bhwc->tc", xf.abs(), gref.abs())
    amb = ((pr["cand"].sum(-1) > 1) & ~pr["exact"]) | amb_relu
    xmax = pw_.abs().amax(-1)                                                   # [B, Hq, Wq, 9]
    allow_w = torch.einsum("bhwt,bhwc->tc", 2 * xmax, torch.where(amb, d.abs(), zero))
    db, sdb = gref.reshape(-1, 64).sum(0), gref.reshape(-1, 64).abs().sum(0)
    allow_b = torch.where(amb_relu, d.abs(), zero).reshape(-1, 64).sum(0)
    return (dw.reshape(3, 3, 1, 64), sdw.reshape(3, 3, 1, 64), allow_w.reshape(3, 3, 1, 64)), (db, sdb, allow_b)


# ------------------------------------------------------------------------------------------------------------------------ checks --
def bound(ref, S, rel, absf, extra=None):
    b = rel * ref.abs() + absf * S
    return b if extra is None else b + extra


def ratio(got, ref, bound):
    """worst |got - ref| / bound over a tensor; an element with a zero bound must match exactly, a non-finite one never does (ratio inf)."""
    got = got.to(torch.float64)
    err = (got - ref).abs()
    bad = ~torch.isfinite(got)
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(bad, torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def check_mask(mask, pr, what):
    """the mask bytes of a fused pool against pool_ref: only bits 0..2; the position inside the clipped window; bit 4 set exactly when the
    maximum is > 0 unless |max| is within the bound; the position the reference's first maximum, any near-tie candidate where the window's
    candidates are not an exact tie -- and an exact tie taken at its FIRST position.  -> (number of near-tie windows, of exact ties > 1)."""
    m = mask.to(torch.int64)
    assert int((m & ~7).abs().sum()) == 0, "%s: mask bits beyond 0..2" % what
    pos = m & 3
    on = (m & 4) != 0
    n = pr["cand"].shape[-1]
    assert int((pos >= n).sum()) == 0, "%s: mask position beyond the window" % what
    valid = torch.broadcast_to(pr["valid"][None, :, :, None, :], pr["cand"].shape)
    inside = torch.gather(valid, -1, pos[..., None])[..., 0]
    bad = ~inside
    assert int(bad.sum()) == 0, "%s: %d mask positions in the padding, first at %s" % (what, int(bad.sum()), bad.nonzero()[0].tolist())
    pm, bd = pr["pre_max"], pr["bound"]
    wrong_on = (on & (pm < -bd)) | (~on & (pm > bd))
    assert int(wrong_on.sum()) == 0, "%s: %d ReLU bits wrong, first at %s" % (what, int(wrong_on.sum()), wrong_on.nonzero()[0].tolist())
    # the position matters only where the gradient passes; the kernels write it everywhere, and where the maximum is exactly 0 it still has to
    # be the first of an exact tie
    first_ok = pos == pr["first"]
    in_cand = torch.gather(pr["cand"], -1, pos[..., None])[..., 0]
    bad_exact = pr["exact"] & ~first_ok
    assert int(bad_exact.sum()) == 0, "%s: %d exact ties not at their first position, first at %s (mask %d, first %d)" % (
        what, int(bad_exact.sum()), bad_exact.nonzero()[0].tolist(), int(pos[bad_exact][0]), int(pr["first"][bad_exact][0]))
    bad_cand = ~pr["exact"] & ~in_cand
    assert int(bad_cand.sum()) == 0, "%s: %d positions that are no maximum, first at %s" % (what, int(bad_cand.sum()), bad_cand.nonzero()[0].tolist())
    ties = pr["exact"] & (pr["cand"].sum(-1) > 1)
    return int((~pr["exact"] & (pr["cand"].sum(-1) > 1)).sum()), int(ties.sum())
