"""The MX oracle (tests/mx_ref.py) against torch's own conversions, hand-worked blocks and the reference's accuracy bar.  CPU only."""
import numpy as np
import pytest
import torch

import mx_ref as M
from oracle.bf16 import f32_to_bf16_bits_rne

FP8 = {"mx_fp8_e4m3": torch.float8_e4m3fn, "mx_fp8_e5m2": torch.float8_e5m2}


def _bits(vals):
    return f32_to_bf16_bits_rne(np.asarray(vals, np.float32))


@pytest.mark.parametrize("mode", sorted(FP8))
def test_fp8_element_conversion_matches_torch(mode):
    """Every float32 inside +-max rounds to the code torch's float32 -> float8 cast gives (torch does not saturate: values beyond max
    are left out)."""
    f = M.FORMATS[mode]
    rng = np.random.default_rng(7)
    # all codes' values, the midpoints between neighbours (ties), and random values over the whole range incl. subnormals
    codes = np.arange(256, dtype=np.uint8)
    vals = M.decode(codes, f)
    vals = vals[np.isfinite(vals)]
    pos = np.unique(np.abs(vals))
    mids = (pos[1:] + pos[:-1]) / 2
    rnd = np.ldexp(rng.random(20000) + 0.5, rng.integers(-20, int(np.log2(f.max)) + 1, 20000)) * rng.choice([-1, 1], 20000)
    cand = np.concatenate([vals, mids, -mids, rnd, [0.0, -0.0]]).astype(np.float32)
    cand = cand[np.abs(cand.astype(np.float64)) <= f.max]
    want = torch.from_numpy(cand).to(FP8[mode]).view(torch.uint8).numpy()
    got = M.encode(cand.astype(np.float64), f)
    assert np.array_equal(got, want), cand[got != want][:8]
    # decode agrees with torch's float8 -> float32
    dec = M.decode(codes, f)
    fin = np.isfinite(dec)
    assert np.array_equal(dec[fin], torch.from_numpy(codes).view(FP8[mode]).float().numpy().astype(np.float64)[fin])


def test_fp4_codes_and_ties():
    f = M.FORMATS["mx_fp4_e2m1"]
    table = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    for c, v in enumerate(table):
        assert M.decode(np.array([c]), f)[0] == v
        assert M.decode(np.array([c | 8]), f)[0] == -v
        assert M.encode(np.array([v]), f)[0] == c
        assert M.encode(np.array([-v]), f)[0] == (c | 8)
    ties = {0.25: 0, 0.75: 2, 2.5: 4, 5.0: 6, 1.25: 2, 1.75: 4, 3.5: 6}
    for v, c in ties.items():
        assert M.encode(np.array([v]), f)[0] == c, v
        assert M.encode(np.array([-v]), f)[0] == (c | 8), -v
    assert M.encode(np.array([7.0, 100.0, -1e30]), f).tolist() == [7, 7, 15]     # saturation
    assert M.encode(np.array([0.2, -0.2]), f).tolist() == [0, 8]                   # rounds to +-0, sign kept


def _q(block, mode):
    d, s, fin = M.quant_mx_rows(_bits([block]), mode)
    return d[0], int(s[0, 0]), bool(fin[0, 0])


@pytest.mark.parametrize("mode", M.MODES)
def test_hand_worked_blocks(mode):
    f = M.FORMATS[mode]
    fp4 = mode == "mx_fp4_e2m1"

    def codes(d):
        if not fp4:
            return d
        out = np.empty(d.size * 2, np.uint8)
        out[0::2], out[1::2] = d & 0xF, d >> 4
        return out

    sign_bit = 0x8 if fp4 else 0x80
    # all zero (both signs)
    blk = np.zeros(32, np.float32)
    blk[3] = -0.0
    d, s, fin = _q(blk, mode)
    assert s == 0 and fin and codes(d)[3] == sign_bit and np.all(np.delete(codes(d), 3) == 0)
    # bf16 subnormals only: scale 0, every element +-0 with its sign
    sub = np.ldexp(np.arange(1, 33, dtype=np.float64), -133).astype(np.float32) * np.where(np.arange(32) % 2, -1, 1)
    d, s, fin = _q(sub, mode)
    assert s == 0 and np.array_equal(codes(d), np.where(np.arange(32) % 2, sign_bit, 0).astype(np.uint8))
    # subnormals next to a normal: the normal's exponent sets the scale, the subnormals go to +-0
    mix = sub.copy()
    mix[5] = 1.0
    d, s, _ = _q(mix, mode)
    assert s == max(127 - f.emax, 0)
    c = codes(d)
    assert M.decode(c[5:6], f)[0] * 2.0 ** (s - 127) == 1.0
    assert np.all((c[np.arange(32) != 5] & (sign_bit - 1)) == 0)
    # maximum at 2^emax * 1.99 (rounds to 1.9921875 in bf16): scale byte 127, the element saturates to max
    big = np.zeros(32, np.float32)
    big[0], big[1] = 2.0 ** f.emax * 1.99, -(2.0 ** f.emax) * 1.99
    d, s, _ = _q(big, mode)
    assert s == 127
    assert M.decode(codes(d)[:2], f).tolist() == [f.max, -f.max]
    # maximum at 2^-120 (FP8: s clamped to 0, the element is x * 2^127) and at 2^-126 (clamped in every format)
    for ex in (-120, -126):
        tiny = np.zeros(32, np.float32)
        tiny[7] = 2.0 ** ex
        d, s, _ = _q(tiny, mode)
        assert s == max(ex + 127 - f.emax, 0)
        assert M.decode(codes(d)[7:8], f)[0] == min(2.0 ** (ex + 127 - s), f.max)
    assert max(-120 + 127 - f.emax, 0) == 0 or fp4
    # maximum at 2^127: s = 254 - emax
    huge = np.zeros(32, np.float32)
    huge[31] = 2.0 ** 127
    d, s, _ = _q(huge, mode)
    assert s == 254 - f.emax and M.decode(codes(d)[31:32], f)[0] == 2.0 ** f.emax
    # Inf / NaN: scale 0xFF, block marked unspecified; the neighbouring block is untouched
    for bad in (np.inf, -np.inf, np.nan):
        row = np.ones(64, np.float32)
        row[40] = bad
        d, s, fin = M.quant_mx_rows(_bits([row]), mode)
        assert s.tolist() == [[127 - f.emax, 0xFF]] and fin.tolist() == [[True, False]]
        dd, ss, _ = M.quant_mx_rows(_bits([row[:32]]), mode)
        assert np.array_equal(d[0, :dd.shape[1]], dd[0]) and ss[0, 0] == s[0, 0]


@pytest.mark.parametrize("mode,bar", [("mx_fp8_e4m3", 2e-3), ("mx_fp8_e5m2", 2e-3), ("mx_fp4_e2m1", 4e-2)])
def test_accuracy_bar_of_the_reference(mode, bar):
    rng = np.random.default_rng(11)
    xb = _bits(rng.standard_normal((64, 7168)).astype(np.float32) * 2)
    d, s, fin = M.quant_mx_rows(xb, mode)
    assert fin.all()
    y = M.dequant_mx_rows(d, s, mode)
    assert M.calc_diff(y, M.bf16_bits_to_f64(xb)) < bar


def test_dispatch_oracle_is_quantise_then_route():
    import mp_workers
    W, T, H, K, E = 2, 24, 64, 4, 8
    xs, idxs, _ = mp_workers.make_inputs(W, T, H, K, E, 0.2)
    for mode in M.MODES:
        per = M.mx_dispatch(xs, idxs, E, mode)
        for r, d, s, fin in per:
            n = r.total_recv
            tri = r.recv_src_idx[:3 * n].reshape(n, 3)
            for j in range(n):
                src, t = int(tri[j, 0]), int(tri[j, 1])
                dd, ss, _ = M.quant_mx_rows(xs[src][t:t + 1], mode)
                assert np.array_equal(d[j], dd[0]) and np.array_equal(s[j], ss[0])
