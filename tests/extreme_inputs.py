"""Inputs at the 16-bit edges of HM's quantisers and inverse transform, and counters that prove a test reached them.

No GPU dependency.  Three parts:
  * saturating residuals and pictures: blocks of 0 and 2^B - 1 side by side (plus light noise, ramps and basis-sign patterns at
    full amplitude), so that a block predicts from neighbours of the opposite value and its low-frequency coefficients approach
    2^15 -- at QP_Y = -QpBdOffset the flat quantiser then clips (TComTrQuant.cpp:1256-1258) and RDOQ's Int levels exceed 32767;
  * synthetic level blocks for the decoder direction: all zero, one extreme level, dense full-range int16, a column of
    same-signed maxima that overflows the first inverse stage, values outside int16;
  * edge counters: int64 restatements of the reference's arithmetic that say how many blocks (or positions) hit each edge.
"""
import numpy as np

INT16_MIN, INT16_MAX = -32768, 32767
QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564)  # g_quantScales (TComRom.cpp)
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)  # g_invQuantScales


def qp_bd_offset(B):
    return 6 * (B - 8)


# ---- saturating residuals / pictures -------------------------------------------------------------------------------------------

def _basis_signs(N, k, l):
    """The sign pattern of DCT basis (k, l) at full amplitude: +-1 per sample."""
    n = np.arange(N)
    row = np.where(np.cos(np.pi * (2 * n + 1) * k / (2 * N)) >= 0, 1, -1)
    col = np.where(np.cos(np.pi * (2 * n + 1) * l / (2 * N)) >= 0, 1, -1)
    return np.outer(col, row)


RESIDUAL_KINDS = ("dc", "dc_neg", "basis", "checker", "halves", "noisy_max")


def saturating_residual(rng, N, B, kind):
    """One N x N residual block whose transform holds coefficients near +-2^15 (int16)."""
    mx = (1 << B) - 1
    if kind == "dc":  # a flat block predicted from the opposite value: DC ~ N * mx * 2^(15 - B - log2 N) ~ 2^15
        r = np.full((N, N), mx, np.int64) - rng.integers(0, 3, (N, N))
    elif kind == "dc_neg":
        r = -np.full((N, N), mx, np.int64) + rng.integers(0, 3, (N, N))
    elif kind == "basis":  # one low-frequency basis at full amplitude, with some energy spread around it
        k, l = int(rng.integers(0, min(N, 4))), int(rng.integers(0, min(N, 4)))
        r = mx * _basis_signs(N, k, l) - np.sign(_basis_signs(N, k, l)) * rng.integers(0, 3, (N, N))
    elif kind == "checker":  # the highest frequency at full amplitude
        r = mx * np.where((np.add.outer(np.arange(N), np.arange(N)) & 1) == 0, 1, -1)
    elif kind == "halves":  # a ramp over a step: several non-zero levels per coefficient group
        r = np.where(np.arange(N)[None, :] < N // 2, mx, -mx) * np.ones((N, 1), np.int64)
        r = r - np.sign(r) * (np.arange(N)[:, None] * mx // (4 * N))
    else:  # noisy_max: |r| near mx with random signs per 2x2 cell, biased to one sign
        s = np.where(rng.random((N, N)) < 0.8, 1, -1)
        r = s * (mx - rng.integers(0, max(2, mx // 16), (N, N)))
    return np.clip(r, -mx, mx).astype(np.int16)


def saturating_picture(rng, w, h, B, scale=16):
    """A 4:2:0 picture of square tiles of 0 and 2^B - 1 at `scale` luma samples (chroma at half), with light noise and
    ramps inside the tiles, and a few full-amplitude checkerboards: every block predicts from neighbours of the opposite value."""
    mx = (1 << B) - 1
    out = []
    for pw, ph, sc in ((w, h, scale), (w // 2, h // 2, max(2, scale // 2)), (w // 2, h // 2, max(2, scale // 2))):
        ty, tx = np.arange(ph)[:, None] // sc, np.arange(pw)[None, :] // sc
        hi = ((ty + tx) & 1) == 0
        noise = rng.integers(0, 1 + max(1, mx // 64), (ph, pw))
        ramp = (np.arange(pw)[None, :] % sc) * max(1, mx // 256)
        p = np.where(hi, mx - noise - ramp, noise + ramp)
        # a few tiles become full-amplitude checkerboards (highest frequency at full swing)
        cells = rng.random(((ph + sc - 1) // sc, (pw + sc - 1) // sc)) < 0.15
        chk = cells[ty, tx] & (((np.arange(ph)[:, None] + np.arange(pw)[None, :]) & 1) == 1)
        p = np.where(chk, mx - p, p)
        out.append(np.clip(p, 0, mx).astype(np.int16))
    return out


# ---- synthetic levels (decoder direction) --------------------------------------------------------------------------------------

LEVEL_KINDS = ("zero", "one_max", "one_min", "dense", "column", "wide")


def synthetic_levels(rng, N, kind):
    """One N x N block of levels (int32, the TCoeff of hmx_levels) for the decoder direction."""
    lv = np.zeros((N, N), np.int64)
    if kind == "one_max":
        lv[rng.integers(0, N), rng.integers(0, N)] = int(rng.choice([INT16_MAX, -INT16_MAX]))
    elif kind == "one_min":
        lv[rng.integers(0, N), rng.integers(0, N)] = INT16_MIN
    elif kind == "dense":
        lv = rng.integers(INT16_MIN, INT16_MAX + 1, (N, N))
    elif kind == "column":
        # a column of same-signed maxima in the low vertical frequencies: the column sum of the first inverse stage overflows
        c = int(rng.integers(0, N))
        s = int(rng.choice([1, -1]))
        lv[:, c] = s * INT16_MAX
        lv[:, (c + 1) % N] = s * (INT16_MAX - rng.integers(0, 64, N))
    elif kind == "wide":  # outside int16: hmx_coeff is int32, the reference clips before de-quantising
        vals = np.array([40000, -40000, 2 ** 31 - 1, -2 ** 31, 65536, -65537, INT16_MAX + 1, INT16_MIN - 1], np.int64)
        lv = rng.integers(-300, 301, (N, N))
        idx = rng.choice(N * N, size=min(N * N, 8), replace=False)
        lv.reshape(-1)[idx] = vals[:len(idx)]
    return lv.astype(np.int32)


# ---- edge counters -------------------------------------------------------------------------------------------------------------

def flat_levels_unclipped(coef, N, B, per, rem, intra_slice=True):
    """The flat quantiser's levels before the clip (TComTrQuant.cpp:1250-1258), int64."""
    c = np.asarray(coef, np.int64).reshape(-1)
    qbits = 14 + per + (15 - B - int(np.log2(N)))
    add = (171 if intra_slice else 85) << (qbits - 9)
    lv = (np.abs(c) * QUANT_SCALES[rem] + add) >> qbits
    return np.where(c < 0, -lv, lv)


def count_flat_clip(coef, N, B, per, rem, intra_slice=True):
    """Positions whose flat level leaves [-32768, 32767]."""
    lv = flat_levels_unclipped(coef, N, B, per, rem, intra_slice)
    return int(np.count_nonzero((lv > INT16_MAX) | (lv < INT16_MIN)))


def count_sbh_on_clipped(lev_sbh, lev_plain):
    """Blocks (or positions) where sign hiding changed a level that the clip had left at 32767 or -32768 -- there the
    reference uses finalChange = -1 (TComTrQuant.cpp:1076-1081).  Compare the same call with sign hiding on and off."""
    a, b = np.asarray(lev_sbh, np.int64), np.asarray(lev_plain, np.int64)
    return int(np.count_nonzero((a != b) & ((b == INT16_MAX) | (b == INT16_MIN))))


def count_dequant_wrap(levels, N, B, per, rem):
    """Positions whose 32-bit de-quantiser product wraps: clip(level) * (invScale << per) + add leaves Int
    (TComTrQuant.cpp:1346-1353)."""
    lv = np.clip(np.asarray(levels, np.int64).reshape(-1), INT16_MIN, INT16_MAX)
    shift = 20 - 14 - (15 - B - int(np.log2(N)))
    p = lv * (INV_QUANT_SCALES[rem] << per) + (1 << (shift - 1))
    return int(np.count_nonzero((p >= 2 ** 31) | (p < -2 ** 31)))


def dequant_int64(levels, N, B, per, rem):
    """xDeQuant without the 32-bit wrap (what it would give with wide arithmetic); compare with the real output to count wraps."""
    lv = np.clip(np.asarray(levels, np.int64).reshape(-1), INT16_MIN, INT16_MAX)
    shift = 20 - 14 - (15 - B - int(np.log2(N)))
    v = (lv * (INV_QUANT_SCALES[rem] << per) + (1 << (shift - 1))) >> shift
    return np.clip(v, INT16_MIN, INT16_MAX)


def transform_matrix(N, dst=False):
    """g_aiT4/8/16/32 or g_as_DST_MAT_4 (rows = basis functions) as int64, built by the oracle."""
    import ctypes as C  # noqa: F401  (the oracle is a ctypes library)
    import oracle_lib as ol
    m = np.zeros(N * N, np.int16)
    if dst:
        ol.oracle().hmo_dst_matrix(m)
    else:
        ol.oracle().hmo_dct_matrix(N, m)
    return m.reshape(N, N).astype(np.int64)


def count_first_stage_clip(deq, N, dst=False):
    """Outputs of the first inverse stage (column transform, shift 7, TComTrQuant.cpp:378, 474-499) that the normative clip
    to 16 bits changes.  deq = the de-quantised coefficients (xDeQuant output), N x N row-major."""
    M = transform_matrix(N, dst)
    c = np.asarray(deq, np.int64).reshape(N, N)
    s = (M.T @ c + 64) >> 7
    return int(np.count_nonzero((s > INT16_MAX) | (s < INT16_MIN)))


def search_sbh_on_clip(rng, N, B, n_want=3, max_tries=600):
    """Residual blocks on which the oracle's flat quantiser lands sign hiding on a clipped level (luma, intra slice, per 0 or 1):
    a random search over saturating residuals, since which position sign hiding picks depends on every rounding remainder of
    the group.  Returns [(residual, qp_y, intra direction)], at most n_want (fewer when the shape cannot clip)."""
    import oracle_lib as ol
    O = ol.oracle()
    bd = qp_bd_offset(B)
    found = []
    for _ in range(max_tries):
        kind = ("dc", "dc_neg", "basis", "checker")[int(rng.integers(0, 4))]
        resi = saturating_residual(rng, N, B, kind)
        qpy, mode = -bd + int(rng.integers(0, 12)), int(rng.integers(0, 35))
        q = O.hmo_setQPforQuant(qpy, 0, bd, 0)
        tmode = mode
        scan = O.hmo_coef_scan_idx(N, 1, 1, mode)
        on, _ = ol.o_transformNxN(resi, N, B, tmode, 0, ol.quant_cfg(q.per, q.rem, 1, 1, scan))
        off, _ = ol.o_transformNxN(resi, N, B, tmode, 0, ol.quant_cfg(q.per, q.rem, 1, 0, scan))
        if count_sbh_on_clipped(on, off):
            found.append((resi, qpy, mode))
            if len(found) >= n_want:
                break
    return found
