"""CPU: the references of the exact C5 delta step (tests/refine_exact.py) checked against each other,
against the scipy oracle and against mpmath, and the bars of tests/test_gpu_refine_exact.py shown to bite:
every corruption of refine_exact.CORRUPTIONS applied to the float64 yardstick, with the factor by which
it misses each bar (printed; DESIGN §2 quotes them).  No GPU."""
import math

import numpy as np
import pytest

import refine_exact as X
from band_signals import LD_OK, LD_REASON
from meteorgpu import _lib
from oracle import iq_oracle as Q

pytestmark = pytest.mark.skipif(not LD_OK, reason=LD_REASON)

FS = 192000.0
# (N, hop, band, noise): C5 (9 needed bins: one in the digit-lane tile), 10 bins, 8 bins with R = 2, an
# empty noise band with one band bin (3 needed bins)
GEOMS = [
    (4096, 1024, (21, 22), (-65, -63)),
    (4096, 1024, (100, 102), (-300, -298)),
    (2048, 1024, (511, 512), (-700, -699)),
    (4096, 1024, (21, 21), (0, -1)),
]
NFR = 6


def _f(v):
    return np.asarray(v, dtype=np.float64)


@pytest.fixture(scope="module")
def cases():
    """{(geometry index, class): (plan, x, frames, truth, quantised, yardstick, amp)}, computed once"""
    out = {}
    for g, (N, hop, band, noise) in enumerate(GEOMS):
        P = X.Plan(N, hop, FS, band, noise)
        assert P.i8()
        fr = list(range(NFR))
        for name, x in X.signals(P, NFR, seed=g).items():
            out[g, name] = (P, x, fr, X.truth(P, x, fr), X.quantised(P, x, fr), X.yardstick(P, x, fr), X.amp(P, x, fr))
    return out


def test_plan_restates_the_library():
    for N, hop, band, noise in GEOMS + [(4096, 1024, (19, 23), (-67, -63)), (1000, 500, (10, 12), (-9, -8))]:
        P = X.Plan(N, hop, FS, band, noise)
        path = _lib.iq_delta64_path(N, hop, FS, band, noise, _lib.MSD_CI16)
        assert (path == _lib.REFINE_INT8_MFMA) == P.i8(), (N, hop, band, noise)


def test_truth_agrees_with_the_oracle(cases):
    """(a) |delta_truth - delta_oracle| within the reference's documented chain (4 log2 N + 11) u amp
    carried through both bands, plus truth's own error"""
    worst = 0.0
    for (g, name), (P, x, fr, (dt, eb, en), _, _, amp) in cases.items():
        z = X._pairs(x)
        f = FS / P.N
        bands = [((lo - 0.3) * f, (hi + 0.3) * f) if hi >= lo else (1.0, 0.0) for lo, hi in (P.band, P.noise)]
        ref = Q.proc_iq_ref(z[:, 0], z[:, 1], FS, bands[0], bands[1], P.N, P.N - P.hop,
                            flag_adaptive_threshold=False)[4]
        assert len(ref) == NFR
        _, _, reference = X.chains(P, _lib.MSD_CI16)
        bar = X.delta_bar(P, _f(eb), _f(en), reference * X.U * amp + X.truth_error(P, amp))
        live = amp > 0
        assert np.isfinite(bar[live]).all(), (g, name)
        r = np.abs(_f(dt) - ref)[live] / bar[live]
        assert (r <= 1.0).all(), (g, name, float(r.max()))
        worst = max(worst, float(r.max(initial=0.0)))
    print(f"\nrefine_exact (a) truth against the scipy oracle: largest ratio to the reference's chain {worst:.4f}")


def test_quantised_within_the_twiddle_term(cases):
    """(b) |sqrt E_quantised - sqrt E_truth| <= sqrt n 91 u amp (+ truth's own error) per band, every class"""
    worst = {}
    for (g, name), (P, x, fr, (_, ebt, ent), (_, ebq, enq), _, amp) in cases.items():
        for n, et, eq in ((P.nb, ebt, ebq), (P.nn, ent, enq)):
            if n == 0:
                continue
            bar = math.sqrt(n) * (_lib.REFINE_I8_CHAIN_QUANT * X.U * amp + X.truth_error(P, amp))
            err = np.abs(_f(np.sqrt(eq) - np.sqrt(et)))
            live = amp > 0
            assert (err[live] <= bar[live]).all(), (g, name)
            assert (err[~live] == 0).all()
            worst[name] = max(worst.get(name, 0.0), float((err[live] / bar[live]).max(initial=0.0)))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
    print("\nrefine_exact (b) quantised against truth, largest ratios to sqrt n 91 u amp: "
          + ", ".join(f"{k} {v:.4f}" for k, v in top))


def test_yardstick_within_the_combination_bar(cases):
    """(c) |sqrt E_yardstick - sqrt E_quantised| <= sqrt n (own - 91 + combine) u amp + 3 u sqrt E per band"""
    worst = 0.0
    for (g, name), (P, x, fr, _, (_, ebq, enq), (_, eby, eny), amp) in cases.items():
        own, combine, _ = X.chains(P, _lib.MSD_CI16)
        assert own == 119.0 and combine == P.R + 12.0
        for n, eq, ey in ((P.nb, ebq, eby), (P.nn, enq, eny)):
            if n == 0:
                assert (ey == 0).all()
                continue
            bar = X.sqrtE_bar(P, n, ey, amp, own, combine)
            err = np.abs(np.sqrt(ey) - _f(np.sqrt(eq)))
            live = amp > 0
            assert (err[live] <= bar[live]).all(), (g, name, float((err[live] / bar[live]).max()))
            worst = max(worst, float((err[live] / bar[live]).max(initial=0.0)))
    print(f"\nrefine_exact (c) yardstick against quantised: largest ratio to the combination bar {worst:.4f}")


def test_library_integers_against_mpmath():
    """(d) msd_i8_coeffs kind 2 within one unit of the correctly rounded round(cos / sin 2^46)"""
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    differ = total = 0
    for N, ks in ((4096, (2, 21, 1024, 2047, 4094, 4031)), (1024, (2, 511)), (3072, (1000,)), (5120, (5118,)),
                  (8192, (4095, 2731))):
        for k in ks:
            for part in (0, 1):
                T = _lib.i8_coeffs(_lib.I8_REFINE, 1024 if k == 21 else 256, N, k, part)
                for n, t in enumerate(T):
                    a = 2 * mp.pi * ((k * n) % N) / N
                    want = int(mp.nint((mp.sin(a) if part else mp.cos(a)) * 2 ** 46))
                    assert abs(int(t) - want) <= 1, (N, k, part, n)
                    differ += int(t) != want
                    total += 1
            assert _lib.i8_coeffs(_lib.I8_REFINE, 4, N, k, 0)[0] == 2 ** 46
    print(f"\nrefine_exact (d) {total} integers against mpmath: {differ} differ from the correctly rounded value")


def test_coeffs_argument_checks():
    for args in ((2, 0, 4096, 3, 0), (2, 1025, 4096, 3, 0), (2, 256, 4096, 4096, 0), (2, 256, 4096, -1, 0),
                 (2, 256, 4096, 3, 2), (3, 256, 4096, 3, 0)):
        T = np.zeros(2048, np.int64)
        rc = _lib.load().msd_i8_coeffs(args[0], None, args[1], args[2], args[3], args[4], _lib.ptr(T))
        assert rc == _lib.MSD_ERR_INVALID, args
        assert not T.any()
    assert _lib.load().msd_i8_coeffs(2, None, 256, 4096, 3, 0, None) == _lib.MSD_ERR_INVALID


def test_every_bound_is_finite(cases):
    """(e) every bar and the restated ed are finite on every frame that is not all zero"""
    for (g, name), (P, x, fr, (_, ebt, ent), _, (_, eby, eny), amp) in cases.items():
        own, combine, reference = X.chains(P, _lib.MSD_CI16)
        live = amp > 0
        assert live.all() == (name != "const0")
        ad = X.amp_device(P, x, fr)
        assert (ad >= amp).all()
        e = X.ed(P, eby, eny, ad, own + combine + reference)
        b1 = X.delta_bar(P, _f(ebt), _f(ent), (own + combine) * X.U * amp + X.truth_error(P, amp))
        b2 = X.delta_bar(P, eby, eny, (own - 91.0 + combine) * X.U * amp)
        for v in (e, b1, b2):
            assert np.isfinite(v[live]).all() and (v > 0).all(), (g, name)
        assert (e >= b1).all()


# ----------------------------------------------------------------------------- (f) the bars bite
BLIND = ()  # corruptions that pass every bar (none: every one below misses at least one)


def _factors(P, x, fr, corrupt, where=None):
    """by what factor the corrupted yardstick misses each bar: {bar: largest err / bar over the frames}"""
    own, combine, _ = X.chains(P, _lib.MSD_CI16)
    amp = X.amp(P, x, fr)
    dt, ebt, ent = X.truth(P, x, fr)
    dq, ebq, enq = X.quantised(P, x, fr)
    dy, _, _ = X.yardstick(P, x, fr)
    dc, ebc, enc = X.yardstick(P, x, fr, corrupt, where)
    out = {}
    b1 = X.delta_bar(P, _f(ebt), _f(ent), (own + combine) * X.U * amp + X.truth_error(P, amp))
    out["model"] = float((np.abs(dc - _f(dt)) / b1).max())
    r = 0.0
    for n, eq, ec in ((P.nb, ebq, ebc), (P.nn, enq, enc)):
        if n:
            r = max(r, float((np.abs(np.sqrt(ec) - _f(np.sqrt(eq))) / X.sqrtE_bar(P, n, ec, amp, own, combine)).max()))
    out["restatement"] = r
    b2 = X.delta_bar(P, _f(ebq), _f(enq), (own - 91.0 + combine) * X.U * amp)
    out["restatement_delta"] = float((np.abs(dc - _f(dq)) / b2).max())
    out["precision"] = X.rms_ld(dc, dq) / (4.0 * X.rms_ld(dy, dq))
    return out


@pytest.mark.parametrize("corrupt", X.CORRUPTIONS)
def test_the_bars_bite(corrupt):
    """(f) each corruption on noise-like input at C5's geometry (9 bins) and with an empty noise band (3
    bins): the factor by which it misses the model bar (truth), the restatement bar (sqrt E per band, and
    carried through delta where E cannot be recovered) and the precision bar (rms over 4 yardsticks)"""
    seen = {}
    for N, hop, band, noise in (GEOMS[0], GEOMS[3]):
        P = X.Plan(N, hop, FS, band, noise)
        fr = list(range(4, 15))
        x = X.signals(P, 16, seed=5)["noise300"]
        f = _factors(P, x, fr, corrupt, where=[3, 7])
        for k, v in f.items():
            seen[k] = max(seen.get(k, 0.0), v)
        print(f"\nrefine_exact (f) {corrupt} nk {P.nk}: " + ", ".join(f"{k} x{v:.3g}" for k, v in f.items()))
    caught = [k for k, v in seen.items() if v > 1.0]
    if corrupt in BLIND:
        assert not caught, (corrupt, seen)
    else:
        assert "restatement" in caught and "restatement_delta" in caught, (corrupt, seen)


def test_the_clean_yardstick_passes_every_bar():
    for N, hop, band, noise in (GEOMS[0], GEOMS[3]):
        P = X.Plan(N, hop, FS, band, noise)
        x = X.signals(P, 16, seed=5)["noise300"]
        f = _factors(P, x, list(range(4, 15)), None)
        assert all(v <= 1.0 for v in f.values()), f
