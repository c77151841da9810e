"""CPU: the restatement of the two int8 matrix-core band kernels (tests/i8_exact.py) is itself held
to what the suite already asserts of them, and shown to catch what the flat 1e-9 dB bar lets through.

* The restated components stay within the asserted bounds of the long-double DFT on the existing
  CPU cases (block: 0.26 u sum|x| and margin._i8_chain; Welch: 1.5 u sum|x| and margin.I8_WELCH).
* The library's coefficients (msd_i8_coeffs, what the plans are built from) lie within one unit of
  the numpy restatements in test_gpu_block_i8.py / test_gpu_welch_i8.py (those reduce the angle
  differently and round half to even, so equality is not asserted), the Welch ones sum to zero, and
  every T fits seven balanced digits.
* The bars bite: the restatement is corrupted five ways (the least-significant digit dropped, the
  two lowest digits' weights exchanged, a K step of 64 samples dropped, two fragment bytes swapped,
  an int32 pair wrapped modulo 2^32); each one's miss factor against the new bars (block: the dB
  bound of i8_exact.block_db_bound; Welch: bit equality, so the factor is the difference in units of
  u relative) is printed beside whether the old |dB| <= 1e-9 bar would have passed it.  The two digit
  corruptions pass the old bar and fail the new ones.  (The wrapped pair is a Welch corruption only:
  the block kernel combines its accumulators in float64, it has no int32 pairs.)
* On every adversarial input of the GPU tests the restated accumulator pairs |a_w| + 256 |a_(w+1)|
  stay below 2^31 wherever the plan combines them in int32; the largest fraction reached is printed."""
import numpy as np
import pytest

import i8_exact as X
from meteorgpu import _lib, dsp
from meteorgpu import margin as M
from test_gpu_block_i8 import _angles
from test_gpu_welch_i8 import PI_LD, _coeffs, _zero_sum_round


def _cpu_input(case, L, rng):
    if case == "noise":
        x = rng.normal(0, 1000, L)
    elif case == "noise300":
        x = rng.normal(0, 300, L)
    elif case == "full_scale":
        x = rng.choice([-32768, 32767], L)
    elif case == "dc":
        x = 30000 + rng.normal(0, 3, L)
    else:
        x = 25000 + rng.normal(0, 5, L)
    return np.clip(np.round(x), -32768, 32767).astype(np.int64)


# ----------------------------------------------------------------------------- within the asserted bounds
@pytest.mark.parametrize("case", ["noise", "full_scale", "dc"])
def test_block_restatement_within_i8_chain(case):
    """test_gpu_block_i8.test_quantised_dft_within_i8_chain's cases and bounds, on the restated
    float64 components (the Horner roundings included)"""
    rng = np.random.default_rng({"noise": 1, "full_scale": 2, "dc": 3}[case])
    B, nfft = 9600, 1024
    L = min(B, nfft)
    x = _cpu_input(case, L, rng)
    w = np.hanning(B)[:L]
    S = float(np.abs(x).max()) * float(w.sum())
    chain = M._i8_chain(L, 5, float(w.sum()))
    absx = float(np.abs(x).sum())
    for band in ((0, 1), (21, 22), (63, 65), (512, 512)):
        plan = X.BlockI8(w, nfft, band, (0, -1))
        p = plan.components(x[None, :])[0]
        for j, k in enumerate(plan.bins):
            ang = _angles(k, L, nfft)
            xw = x.astype(np.longdouble) * w.astype(np.longdouble)
            ex_re, ex_im = np.sum(xw * np.cos(ang)), -np.sum(xw * np.sin(ang))
            err = float(np.hypot(np.longdouble(p[2 * j]) - ex_re, np.longdouble(p[2 * j + 1]) - ex_im))
            assert err <= 0.26 * M.U * absx + 1e-18 * S, (k, err / (M.U * absx))
            assert err <= chain * M.U * S


@pytest.mark.parametrize("case", ["noise300", "dc25000", "full_scale"])
def test_welch_restatement_within_bound(case):
    """test_gpu_welch_i8.test_folded_detrend_quantisation_within_bound's cases and bounds, on the
    restated float64 value v 2^-53 (its single rounding included)"""
    rng = np.random.default_rng({"noise300": 1, "dc25000": 2, "full_scale": 3}[case])
    L, nfft = 256, 4096
    x = _cpu_input(case, L, rng)
    w = np.hanning(L + 1)[:-1]
    absx = float(np.abs(x).sum())
    plan = X.WelchI8(L, L, L // 2, nfft, 1.0, 1.0, [(0, 1), (100, 100), (1024, 1025), (2048, 2048)], w)
    v = plan.sums(x[None, :]).astype(np.float64)[0] * 2.0 ** -53
    xm = x.astype(np.longdouble) - x.astype(np.longdouble).sum() / L
    for j, k in enumerate(plan.bins):
        a = 2 * PI_LD * ((k * np.arange(L, dtype=np.int64)) % nfft).astype(np.longdouble) / np.longdouble(nfft)
        er, ei = np.sum(xm * w * np.cos(a)), -np.sum(xm * w * np.sin(a))
        err = float(np.hypot(np.longdouble(v[2 * j]) - er, np.longdouble(v[2 * j + 1]) - ei))
        assert err <= 1.5 * M.U * absx, (k, err / (M.U * absx))
        assert err <= M.I8_WELCH * M.U * L * float(np.abs(x).max())


# ----------------------------------------------------------------------------- the coefficients
BLOCK_PLANS = [(9600, 1024, 1024), (512, 512, 512), (256, 256, 256), (1024, 1024, 2048)]  # (B, L, nfft)


@pytest.mark.parametrize("B,L,nfft", BLOCK_PLANS)
def test_block_coefficients_near_numpy_and_fit(B, L, nfft):
    w = dsp.hanning_sym(B)[:L]
    scale = np.longdouble(2.0 ** 54)
    for k in (0, 1, 21, 63, nfft // 4, nfft // 2 - 1, nfft // 2):
        a = _angles(k, L, nfft)
        for part, ref in ((0, np.rint(w.astype(np.longdouble) * np.cos(a) * scale)),
                          (1, np.rint(-w.astype(np.longdouble) * np.sin(a) * scale))):
            T = _lib.i8_coeffs(_lib.I8_BLOCK, w, nfft, k, part)
            assert np.abs(T - ref.astype(np.int64)).max() <= 1
            assert X.digits7(T)[1]
            d, _ = X.digits7(T)
            assert np.array_equal(X.undigits(d), T) and d.min() >= -128 and d.max() <= 127


@pytest.mark.parametrize("L,nfft", [(64, 2048), (128, 2048), (192, 1024), (256, 4096), (512, 4096)])
def test_welch_coefficients_near_numpy_sum_to_zero_and_fit(L, nfft):
    w = dsp.hann_periodic(L)
    for k in (0, 1, 100, nfft // 4, nfft // 4 + 1, nfft // 2 - 1, nfft // 2):
        for part, c in enumerate(_coeffs(w, k, nfft)):
            T = _lib.i8_coeffs(_lib.I8_WELCH, w, nfft, k, part)
            assert int(T.sum()) == 0
            assert np.abs(T - np.array(_zero_sum_round(c), dtype=np.int64)).max() <= 1
            d, fits = X.digits7(T)
            assert fits and np.array_equal(X.undigits(d), T)


def test_coefficient_entry_refuses_bad_arguments():
    w = dsp.hann_periodic(64)
    for bad in (lambda: _lib.i8_coeffs(3, w, 64, 0, 0), lambda: _lib.i8_coeffs(0, w, 64, 33, 0),
                lambda: _lib.i8_coeffs(1, w, 64, 0, 2), lambda: _lib.i8_coeffs(0, 1.5 * w, 64, 0, 0)):
        with pytest.raises(_lib.MsdError) as e:
            bad()
        assert e.value.code == _lib.MSD_ERR_INVALID


def test_np_sum_small_is_numpy_order():
    rng = np.random.default_rng(5)
    for n in range(0, 9):
        p = rng.random((50, n)) * 10.0 ** rng.integers(-12, 12, (50, n))
        assert np.array_equal(X.np_sum_small(p), np.array([np.sum(np.ascontiguousarray(r)) for r in p]))


# ----------------------------------------------------------------------------- the bars bite
OLD_BAR = 1e-9


def _block_case():
    B, nfft = 9600, 1024
    L = 1024
    w = dsp.hanning_sym(B)[:L]
    plan = X.BlockI8(w, nfft, (21, 22), (63, 65))
    rng = np.random.default_rng(11)
    x = np.clip(np.round(rng.normal(0, 300, (64, L))), -32768, 32767).astype(np.int64)
    return plan, x


def _welch_case():
    L, nfft, fs = 256, 4096, 4000
    w = dsp.hann_periodic(L)
    scale = 1.0 / (fs * float((w * w).sum()))
    plan = X.WelchI8(800, L, 128, nfft, 1 / 32768, scale, [(870, 972), (1175, 1277)], w)
    rng = np.random.default_rng(12)
    x = np.clip(np.round(rng.normal(0, 300, (16, 800))), -32768, 32767).astype(np.int64)
    return plan, x


def test_mutations_pass_old_bar_and_fail_new(capsys):
    """each corruption's miss factor against the new bars and whether the 1e-9 dB bar sees it"""
    rows = []
    plan, x = _block_case()
    bd, nd, dl = plan.db(x)
    for kind in X.MUTATIONS:
        mb, mn, md = plan.db(x, X.mutate(plan.dig, kind))
        miss = max(float((np.abs(mb - bd) / X.block_db_bound(bd)).max()),
                   float((np.abs(mn - nd) / X.block_db_bound(nd)).max()))
        old = max(float(np.abs(mb - bd).max()), float(np.abs(mn - nd).max()), float(np.abs(md - dl).max()))
        rows.append(("block", kind, miss, old))
    plan, x = _welch_case()
    psd = plan.psd(x)
    db = plan.band_db(psd)
    cases = [(kind, dict(T=X.undigits(X.mutate(plan.dig, kind)))) for kind in X.MUTATIONS]
    cases.append(("wrap_int32_pair", dict(offset=1 << 32)))  # the pair a_0 + 256 a_1 off by 2^32
    for kind, kw in cases:
        m = plan.psd(x, **kw)
        miss = float((np.abs(m - psd) / (M.U * psd)).max())  # bit equality: any difference misses
        old = float(np.abs(plan.band_db(m) - db).max())
        rows.append(("welch", kind, miss, old))
    with capsys.disabled():
        for path, kind, miss, old in rows:
            print(f"\ni8_exact mutation {path:5s} {kind:16s} miss factor {miss:10.3g}  |dB| {old:9.3g} "
                  f"old bar {'passes' if old <= OLD_BAR else 'fails'}", end="")
        print()
    for path, kind, miss, old in rows:
        assert miss > 1.0, (path, kind)  # every corruption misses the new bar
        if kind in ("drop_lsd", "swap_low_weights"):
            assert old <= OLD_BAR, (path, kind, old)  # ... and these two the old bar never saw


# ----------------------------------------------------------------------------- the int32 pairs
WELCH_PAIR_PLANS = [(64, 96, 2048, [(0, 0), (1018, 1024)]), (128, 384, 2048, [(440, 447)]),
                    (192, 480, 1024, [(250, 258)]), (256, 800, 4096, [(870, 972), (1175, 1277), (460, 562)]),
                    (512, 2560, 4096, [(1850, 1858)])]


@pytest.mark.parametrize("L,B,nfft,bands", WELCH_PAIR_PLANS)
def test_pairs_stay_below_2_31_on_adversarial_inputs(L, B, nfft, bands, capsys):
    """wherever the plan's bound lets the kernel combine its accumulators in int32 pairs, the pairs
    restated from the adversarial inputs' own accumulators stay below 2^31 (and below the bound)"""
    w = dsp.hann_periodic(L)
    plan = X.WelchI8(B, L, L // 2, nfft, 1 / 32768, 1.0, bands, w)
    worst = int(np.argmax(plan.pair_bound.max(axis=0)))  # the component closest to the limit
    _, blocks = X.adversarial_blocks(B, L, plan.dig[:, worst], seed=L)
    a = np.abs(plan.accumulators(plan.segments(blocks)))  # [8, R, ncomp]
    pair = np.stack([a[i] + 256 * a[i + 1] for i in range(0, 8, 2)])  # [4, R, ncomp]
    assert (pair.max(axis=1) <= plan.pair_bound).all()
    frac = float(pair.max()) / 2 ** 31
    with capsys.disabled():
        print(f"\ni8_exact pairs nperseg {L}: plan pairs {plan.pairs}, bound {plan.pair_bound.max() / 2 ** 31:.3f} "
              f"of 2^31, reached {frac:.3f}")
    if plan.pairs:
        assert frac < 1.0
    assert plan.pairs == (L < 512)  # nperseg 512 runs the eight-term sum (test_pair_bound_live_default)
    # the exact sum from the accumulators is the sum from T: the offset's term vanishes
    S = plan.sums(plan.segments(blocks))
    acc = plan.accumulators(plan.segments(blocks)).astype(object)
    assert (sum(acc[i] * 256 ** i for i in range(8)) == S).all()
