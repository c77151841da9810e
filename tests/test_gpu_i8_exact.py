"""GPU: the two int8 matrix-core band kernels (csrc/welch_i8.hip, csrc/block_i8.hip) held to their
exact integer sums -- to tests/i8_exact.py's restatement of their arithmetic from the library's own
coefficients -- where test_gpu_welch_i8.py / test_gpu_block_i8.py hold them to |dB - numpy| <= 1e-9.

Welch psd: every existing block bit-equal (np.array_equal) to the restatement, every entry past a
file's blocks still the sentinel, silent and constant blocks exactly 0; nperseg 64-512, 1-16
segments per block (one segment per block: 8 blocks per 16-row tile, which the kernel's averaging
lanes cover), 1-309 bins, a folded and an unfolded sample scale, every form of the kernel
(MSD_OPT_WELCH_I8_FORM) on the adversarial inputs, three files at odd offsets, and two runs whose
waves walk a second tile.  nperseg 320, 384 and 448 (no instantiation: the float64 Goertzel kernel)
run and match scipy within 1e-9 dB.
Welch band dB, from the same launch: |band_db - 10 log10(np.sum(psd_gpu[band]))| <= 4 u (|dB| + 1),
the term margin.band_db_error charges the logarithm, -inf exactly where the sum is 0; every tail
length of both sum paths at MSD_WELCH_MAX_BANDS bands.
Block path (only dB is exposed): |dB_gpu - dB_restated| <= (10 / ln 10) 2 u + 4 u (|dB| + 1) per
band (i8_exact.block_db_bound), delta within both bands' bounds + u |delta|; L 256 / 512 / 1024,
B = L, the cropped window foot (B 9600), zero padding, 1-8 bins with the DC and Nyquist bins, an
empty noise band (exactly 10 log10(1e-12)), files at odd offsets, a partial last tile, and more
tiles than the grid's waves."""
import math

import numpy as np
import pytest

import i8_exact as X
from meteorgpu import margin as M

SENT = -777.0


def _cus():
    """the device's compute units (the kernels size their grids from them)"""
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256  # MI355X


def _layout(blocks, B, pad=16):
    """three files at odd sample offsets: B - 1 samples (no block), the first block alone, the rest
    and one sample more; (buf, offs, lens, the blocks [n, B] of each file)"""
    junk = np.full(B - 1, 1234, np.int16)
    files = [junk, blocks[0], np.concatenate([blocks[1:].reshape(-1), np.array([-5], np.int16)])]
    per = [blocks[:0], blocks[:1], blocks[1:]]
    offs, pos = [], 3
    for f in files:
        offs.append(pos)
        pos += f.size + (2 if (pos + f.size) % 2 else 1)  # the next offset odd again
    buf = np.full(pos + pad, 4321, np.int16)
    for o, f in zip(offs, files):
        assert o % 2 == 1
        buf[o: o + f.size] = f
    return buf, offs, [f.size for f in files], per


# ----------------------------------------------------------------------------- Welch
def _welch_cfg(B, L, noverlap, nfft, sample_scale, bands, fs=4000.0):
    from meteorgpu import _lib, dsp
    win = dsp.hann_periodic(L)
    wc = win.astype(np.complex128)
    c = _lib.MsdWelchCfg()
    c.block_size, c.nperseg, c.noverlap, c.nfft = B, L, noverlap, nfft
    c.sample_scale = sample_scale
    c.scale = float(np.real(1.0 / (fs * (wc * wc).sum())))
    c.nbands = len(bands)
    for j, (lo, hi) in enumerate(bands):
        c.band_lo[j], c.band_hi[j] = lo, hi
    return c, win, X.WelchI8(B, L, noverlap, nfft, sample_scale, c.scale, bands, win)


def _welch_launch(c, win, buf, offs, lens, form=0, ld_extra=2):
    """(psd [nf, ld, nslots], band dB [nf, nbands, ld], blocks per file): every output buffer filled
    with the sentinel before the launch"""
    from meteorgpu import _lib, dsp
    ctx = dsp.context(0)
    B = int(c.block_size)
    nbs = [(n - B) // B + 1 if n >= B else 0 for n in lens]
    nf, max_blocks = len(lens), max(max(nbs), 1)
    ld = max_blocks + ld_extra
    nslots = sum(max(0, int(c.band_hi[j]) - int(c.band_lo[j]) + 1) for j in range(int(c.nbands)))
    nbands = int(c.nbands)
    plan = _lib.WelchPlan(ctx, c, win)
    d_x, d_off, d_len = ctx.alloc(2 * buf.size), ctx.alloc(8 * nf), ctx.alloc(8 * nf)
    d_db, d_psd = ctx.alloc(8 * nf * nbands * ld), ctx.alloc(8 * nf * ld * nslots)
    try:
        d_x.upload(buf)
        d_off.upload(np.array(offs, np.int64))
        d_len.upload(np.array(lens, np.int64))
        d_db.upload(np.full(nf * nbands * ld, SENT))
        d_psd.upload(np.full(nf * ld * nslots, SENT))
        ctx.set_option(_lib.OPT_WELCH_I8_FORM, form)
        plan.run_dev(d_x, np.int16, d_off, d_len, nf, max_blocks, d_db, ld, psd=d_psd)
        ctx.synchronize()
        db = d_db.download(np.empty((nf, nbands, ld), np.float64))
        psd = d_psd.download(np.empty((nf, ld, nslots), np.float64))
    finally:
        ctx.set_option(_lib.OPT_WELCH_I8_FORM, 0)
        plan.close()
        for b in (d_x, d_off, d_len, d_db, d_psd):
            b.free()
    return psd, db, nbs


def _check_welch(R, per, psd, db, nbs, what=""):
    """psd bit-equal to the restatement R on every block of every file, the sentinel past them; the
    band dB within the logarithm's term of np.sum over the kernel's own psd; returns the entries
    compared"""
    count = 0
    for i, blocks in enumerate(per):
        k = nbs[i]
        assert k == len(blocks)
        assert (psd[i, k:] == SENT).all(), (what, i)
        assert (db[i, :, k:] == SENT).all(), (what, i)
        if k == 0:
            continue
        want = R.psd(blocks)
        bad = np.argwhere(psd[i, :k] != want)
        assert np.array_equal(psd[i, :k], want), (what, i, len(bad), bad[:4].tolist())
        count += want.size
        ref = R.band_db(psd[i, :k])
        got = db[i, :, :k]
        zero = np.isneginf(ref)
        assert np.array_equal(np.isneginf(got), zero), (what, i)
        fin = ~zero
        assert np.isfinite(got[fin]).all()
        assert (np.abs(got[fin] - ref[fin]) <= 4.0 * M.U * (np.abs(ref[fin]) + 1.0)).all(), (what, i)
    return count


def _adversarial(R, B, L, seed):
    worst = int(np.argmax(R.pair_bound.max(axis=0)))
    return X.adversarial_blocks(B, L, R.dig[:, worst], seed)


# (nperseg, block size, nfft, sample scale, bands): noverlap nperseg // 2; the segment count follows
WELCH_SHAPES = [
    (64, 64, 2048, 1 / 32768, [(0, 0)]),                                   # 1 segment, 1 slot: the DC bin
    (64, 96, 2048, 1 / 32768, [(1018, 1024)]),                             # 2 segments, 7 slots, Nyquist
    (128, 256, 2048, 1 / 30000, [(440, 447)]),                             # 3 segments, 8 slots, unfolded
    (192, 480, 1024, 1 / 32768, [(250, 255), (300, 302)]),                 # 4 segments, KS 3, 9 slots
    (256, 800, 4096, 1 / 32768, [(870, 972), (1175, 1277), (460, 562)]),   # the live default: 5, 309 slots
    (256, 800, 4096, 1 / 30000, [(870, 876)]),                             # 5 segments unfolded: generic
    (256, 896, 4096, 1 / 30000, [(2042, 2048)]),                           # 6 segments, unfolded
    (512, 2304, 4096, 1 / 32768, [(1850, 1858)]),                          # 8 segments, KS 8 (no pairs)
    (128, 640, 2048, 1 / 32768, [(0, 7)]),                                 # 9 segments
    (64, 512, 2048, 1 / 32768, [(500, 508)]),                              # 15 segments
    (192, 1632, 1024, 1 / 30000, [(511, 511)]),                            # 16 segments, 1 slot
    (256, 300, 4096, 1 / 32768, [(1000, 1007)]),                           # 1 segment, block > nperseg
    (512, 512, 4096, 1 / 32768, [(2000, 2006)]),                           # 1 segment, KS 8
]
WELCH_NSEG = [1, 2, 3, 4, 5, 5, 6, 8, 9, 15, 16, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nseg", list(zip(WELCH_SHAPES, WELCH_NSEG)),
                         ids=[f"L{s[0]}-B{s[1]}-nseg{n}-{'fold' if s[3] == 1 / 32768 else 'nofold'}"
                              for s, n in zip(WELCH_SHAPES, WELCH_NSEG)])
def test_welch_psd_bit_equal_on_adversarial_inputs(shape, nseg):
    L, B, nfft, sscale, bands = shape
    c, win, R = _welch_cfg(B, L, L // 2, nfft, sscale, bands)
    assert R.nseg == nseg and R.fits and R.fold == (sscale == 1 / 32768)
    names, blocks = _adversarial(R, B, L, seed=B + L)
    buf, offs, lens, per = _layout(blocks, B)
    # bit 0: the eight-term digit sum; bit 1: the generic instantiation instead of the 5-segment one
    forms = (0, 1, 2, 3) if (nseg == 5 and R.fold and L == 256) else (0, 1)
    total = 0
    for form in forms:
        psd, db, nbs = _welch_launch(c, win, buf, offs, lens, form)
        total += _check_welch(R, per, psd, db, nbs, what=f"form {form}")
        if form == 0:
            rest = dict(zip(names[1:], psd[2]))
            for name in names[1:]:
                if name == "silence" or name.startswith("const"):
                    assert (rest[name] == 0.0).all(), name  # the detrend removes a constant exactly
    print(f"\ni8_exact welch nperseg {L} block {B} nseg {nseg} slots {R.nslots} fold {R.fold} pairs {R.pairs}: "
          f"{total} psd entries compared over forms {forms}, all equal")


@pytest.mark.gpu
def test_welch_three_files_b_minus_1_b_17b_plus_1():
    """lengths B - 1, B and 17 B + 1 at odd offsets through the live default plan"""
    L, B, nfft = 256, 800, 4096
    c, win, R = _welch_cfg(B, L, 128, nfft, 1 / 32768, [(870, 972), (1175, 1277), (460, 562)])
    rng = np.random.default_rng(3)
    blocks = np.clip(np.round(rng.normal(0, 300, (18, B))), -32768, 32767).astype(np.int16)
    buf, offs, lens, per = _layout(blocks, B)
    assert lens == [B - 1, B, 17 * B + 1]
    psd, db, nbs = _welch_launch(c, win, buf, offs, lens)
    assert nbs == [0, 1, 17]
    n = _check_welch(R, per, psd, db, nbs)
    print(f"\ni8_exact welch three files B - 1, B, 17 B + 1: {n} psd entries compared, all equal")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["generic", "five_segments"])
def test_welch_second_trip(kind):
    """more tiles than wave slots: a wave of every XCD walks a second tile (generic: nperseg 64,
    block 96, tiles of 8 blocks; 5 segments: units of 16 blocks, 2 slots), the smallest such count"""
    cus = _cus()
    if kind == "generic":
        L, B, nfft, bands = 64, 96, 2048, [(300, 300)]
        per_tile = 8
    else:
        L, B, nfft, bands = 256, 800, 4096, [(1000, 1001)]
        per_tile = 16
    c, win, R = _welch_cfg(B, L, L // 2, nfft, 1 / 32768, bands)
    nslot = max(1, cus // 8) * 12  # one column group: reps = CUs per XCD, 12 waves per workgroup
    nblk = (8 * nslot + 8) * per_tile - 3  # every XCD's share one tile more than its wave slots; a partial last
    rng = np.random.default_rng(17)
    x = rng.integers(-900, 901, nblk * B + 5, dtype=np.int16)
    buf = np.concatenate([np.zeros(1, np.int16), x, np.zeros(16, np.int16)])
    psd, db, nbs = _welch_launch(c, win, buf, [1], [x.size])
    assert nbs == [nblk]
    n = _check_welch(R, [x[: nblk * B].reshape(nblk, B)], psd, db, nbs, what=kind)
    print(f"\ni8_exact welch second trip {kind}: {nblk} blocks, {n} psd entries compared, all equal")


@pytest.mark.gpu
@pytest.mark.parametrize("nperseg", [320, 384, 448])
def test_welch_nperseg_without_instantiation_runs(nperseg):
    """nperseg 320, 384 and 448 are multiples of 64 below 512 that the int8 kernel has no
    instantiation for: int16 input runs (the float64 Goertzel kernel) and matches scipy within 1e-9 dB"""
    from scipy.signal import welch
    from meteorgpu import _lib, dsp, synth
    fs, B, nfft = 8000, 1600, 4096
    x, _ = synth.synth_real(seed=nperseg, fs=fs, duration_s=3.0, f0=2000, sigma=400, rate_per_min=30)
    bands = [(973, 1075), (1178, 1280), (767, 869)]
    win = dsp.hann_periodic(nperseg)
    wc = win.astype(np.complex128)
    c = _lib.MsdWelchCfg()
    c.block_size, c.nperseg, c.noverlap, c.nfft = B, nperseg, nperseg // 2, nfft
    c.sample_scale = 1 / 32768
    c.scale = float(np.real(1.0 / (fs * (wc * wc).sum())))
    c.nbands = len(bands)
    for j, (lo, hi) in enumerate(bands):
        c.band_lo[j], c.band_hi[j] = lo, hi
    ctx = dsp.context(0)
    plan = _lib.WelchPlan(ctx, c, win)
    try:
        got = plan.run(np.ascontiguousarray(x))
        ctx.set_option(_lib.OPT_WELCH_GOERTZEL, 1)
        gz = plan.run(np.ascontiguousarray(x))
    finally:
        ctx.set_option(_lib.OPT_WELCH_GOERTZEL, 0)
        plan.close()
    nb = (len(x) - B) // B + 1
    ref = np.empty((3, nb))
    for b in range(nb):
        _, P = welch(x[b * B:(b + 1) * B].astype(np.float64) / 32768.0, fs, nperseg=nperseg, noverlap=nperseg // 2,
                     nfft=nfft)
        for j, (lo, hi) in enumerate(bands):
            ref[j, b] = 10 * np.log10(np.sum(P[lo: hi + 1]))
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)
    assert np.array_equal(got, gz)  # the documented path: the Goertzel kernel


WIDTHS = [[1, 2, 7, 8, 9, 15, 16, 17], [127, 128, 129, 130, 200, 1, 8, 9]]


@pytest.mark.gpu
@pytest.mark.parametrize("widths", WIDTHS, ids=["narrow", "wide"])
def test_welch_band_db_every_width(widths):
    """MSD_WELCH_MAX_BANDS bands of widths 1-200: the single-lane sums (< 8, > 128 bins), the
    eight-lane sum (8-128) and every tail length, against np.sum over the kernel's own psd"""
    from meteorgpu import _lib
    assert len(widths) == _lib.WELCH_MAX_BANDS
    L, B, nfft = 256, 384, 4096
    bands, lo = [], 40
    for w in widths:
        bands.append((lo, lo + w - 1))
        lo += w + 3
    c, win, R = _welch_cfg(B, L, 128, nfft, 1 / 32768, bands)
    assert R.nseg == 2
    rng = np.random.default_rng(sum(widths))
    blocks = np.clip(np.round(rng.normal(0, 300, (11, B))), -32768, 32767).astype(np.int16)
    blocks[4] = 0       # a silent block: every band -inf
    blocks[7] = -129    # a constant block
    buf, offs, lens, per = _layout(blocks, B)
    psd, db, nbs = _welch_launch(c, win, buf, offs, lens)
    n = _check_welch(R, per, psd, db, nbs)
    print(f"\ni8_exact welch band widths {widths}: {n} psd entries compared, all equal; band dB within 4 u (|dB| + 1)")
    assert np.isneginf(db[2][:, 3]).all() and np.isneginf(db[2][:, 6]).all()  # blocks 4 and 7 = rows 3, 6 of file 2


# ----------------------------------------------------------------------------- block path
# (B, nfft, band bins, noise bins): L = min(B, nfft)
BLOCK_SHAPES = [
    (256, 256, (0, 0), (0, -1)),            # L 256 = B, 1 bin: the DC bin; an empty noise band
    (512, 512, (255, 256), (10, 14)),       # L 512 = B, 2 + 5 = 7 bins, the Nyquist bin
    (1024, 1024, (100, 103), (0, 3)),       # L 1024 = B, 8 bins, the DC bin
    (9600, 1024, (21, 22), (63, 65)),       # the cropped window foot (C3)
    (1024, 2048, (1, 1), (1024, 1024)),     # zero padding, 2 bins, the Nyquist bin
]


def _block_launch(B, nfft, band, noise, buf, offs, lens, ld_extra=3):
    from meteorgpu import _lib, dsp
    L = min(B, nfft)
    w = dsp.hanning_sym(B)[:L]
    ctx = dsp.context(0)
    nbs = [n // B for n in lens]
    nf, max_blocks = len(lens), max(max(nbs), 1)
    ld = max_blocks + ld_extra
    plan = _lib.BlockPlan(ctx, B, nfft, w, band, noise)
    d_x, d_off, d_len = ctx.alloc(2 * buf.size), ctx.alloc(8 * nf), ctx.alloc(8 * nf)
    d_out = [ctx.alloc(8 * nf * ld) for _ in range(3)]
    try:
        d_x.upload(buf)
        d_off.upload(np.array(offs, np.int64))
        d_len.upload(np.array(lens, np.int64))
        for d in d_out:
            d.upload(np.full((nf, ld), SENT))
        plan.run_dev(d_x, np.int16, d_off, d_len, nf, max_blocks, *d_out, ld)
        ctx.synchronize()
        got = [d.download(np.empty((nf, ld), np.float64)) for d in d_out]
    finally:
        plan.close()
        for d in (d_x, d_off, d_len, *d_out):
            d.free()
    return got, nbs, X.BlockI8(w, nfft, band, noise)


def _check_block(R, per, got, nbs, what=""):
    """dB and delta within the bar of the restatement; returns the largest ratio to the bound"""
    worst = 0.0
    for i, blocks in enumerate(per):
        k = nbs[i]
        assert k == len(blocks)
        for j in range(3):
            assert (got[j][i, k:] == SENT).all(), (what, i, j)
        if k == 0:
            continue
        bd, nd, dl = R.db(blocks)
        eb, en = X.block_db_bound(bd), X.block_db_bound(nd)
        for g, ref, bound in ((got[0][i, :k], bd, eb), (got[1][i, :k], nd, en),
                              (got[2][i, :k], dl, eb + en + M.U * np.abs(dl))):
            ratio = np.abs(g - ref) / bound
            assert (ratio <= 1.0).all(), (what, i, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
        if R.nnoise == 0:
            assert (got[1][i, :k] == 10.0 * math.log10(1e-12)).all()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("B,nfft,band,noise", BLOCK_SHAPES, ids=[f"B{s[0]}-nfft{s[1]}" for s in BLOCK_SHAPES])
def test_block_db_against_restatement(B, nfft, band, noise):
    """the adversarial inputs in three files at odd offsets (37 blocks: a partial last tile)"""
    from meteorgpu import dsp
    L = min(B, nfft)
    R0 = X.BlockI8(dsp.hanning_sym(B)[:L], nfft, band, noise)
    assert R0.fits
    _, blocks = X.adversarial_blocks(B, L, R0.dig[:, 0], seed=B + nfft)
    buf, offs, lens, per = _layout(blocks, B)
    got, nbs, R = _block_launch(B, nfft, band, noise, buf, offs, lens)
    assert sum(nbs) % 16 != 0
    worst = _check_block(R, per, got, nbs, what=f"B {B} nfft {nfft} bins {len(R.bins)}")
    print(f"\ni8_exact block B {B} nfft {nfft} bins {len(R.bins)}: largest ratio to the bound {worst:.3f}")


@pytest.mark.gpu
def test_block_more_tiles_than_waves():
    """more than 8 num_cu tiles of L = 256 blocks: the grid's waves walk a second tile"""
    B, nfft, band, noise = 256, 512, (37, 37), (0, -1)
    nblk = 16 * (8 * _cus() + 1) + 5
    rng = np.random.default_rng(23)
    x = rng.integers(-900, 901, nblk * B + 7, dtype=np.int16)
    buf = np.concatenate([np.zeros(1, np.int16), x, np.zeros(16, np.int16)])
    got, nbs, R = _block_launch(B, nfft, band, noise, buf, [1], [x.size])
    assert nbs == [nblk]
    worst = _check_block(R, [x[: nblk * B].reshape(nblk, B)], got, nbs, what="second trip")
    print(f"\ni8_exact block second trip {nblk} blocks: largest ratio to the bound {worst:.3f}")
