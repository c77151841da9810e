"""GPU: the C5 I/Q certificate on coloured, degenerate and near-silent input (tests/iq_signals.py).

"Certified" promises the float64 reference's detections (include/msdsp.h).  It
rests on the fp32 path's per-bin error model (IQ_CHAIN, csrc/stream.hip), on the bound ed the band
delta kernel derives from it and from the spectrogram kernel's energy partials, and on the bounds of
the float64 / int8 refinement.  test_gpu_certify.py checks them on white noise of sigma ~1000 with
in-band pings; here every class of iq_signals, against the float64 oracle (computed once per class):

* the premise, every bin of every frame but bins -1, 0, 1:
      |sqrt P_gpu - sqrt P_ref| <= 37 * 2^-24 * sqrt(1.001 S_ref) + 2 * 2^-24 * sqrt P_ref,
  with S_ref the REFERENCE's total power of the frame (not the kernel's partials) and 37 read from
  csrc/stream.hip (IQ_CHAIN: narrowing it there fails this test);
* soundness: |delta_gpu - delta_ref| <= ed on every frame with a finite ed, no tolerance;
* not vacuous: on the white-like classes no frame has ed = +inf and median(ed) < 1e-2 dB;
* the refinement (float64 Goertzel rows, the int8 MFMA step, the int16 Goertzel A/B switch, the
  direct step at hop 1000): |delta - delta_ref| <= ed, ed finite where the reference's band energies
  are non-zero;
* end to end, delta="fp32" and "auto": the refinement loop ends in exactly one of certified /
  near_tie / refine_budget_exhausted; certified means the oracle's detections exactly and its dB
  within 1e-9; an exact tie of delta and threshold at every frame (zeros, a constant) is never
  certified; every class with pings ends certified with detections.

Each test prints its figures (a line starting CERT4 / CERT5 / CERT6): DESIGN.md 4.5c records them.
"""
import functools

import numpy as np
import pytest

import iq_signals as G
from meteorgpu import _lib, iq
from meteorgpu.dsp import context
from meteorgpu.stream import CertifyingShard
from oracle import dsp_oracle as O
from oracle import iq_oracle as Q

pytestmark = pytest.mark.gpu

FS, N, HOP, KW = G.FS, G.N, G.HOP, G.KW
U = 2.0 ** -24
CASES = pytest.mark.parametrize("name,kind", G.CASES, ids=G.CASE_IDS)


def _detector(sg, ctx=None, hop=HOP, delta="fp32"):
    buf, _ = iq.interleave(sg.i, sg.q)
    n = buf.size // 2
    det = iq.IQShardDetector(ctx or context(0), n, FS, N, N - hop, sg.band, sg.noise, 4.0, True, dtype=buf.dtype,
                             certify=True, delta=delta, **KW)
    try:
        det.process_host(buf[2 * det.s0: 2 * det.s1])
        det.synchronize()
    except BaseException:
        det.close()
        raise
    return det


# ------------------------------------------------------------- the fp32 bound and its premise
@CASES
def test_fp32_bound_and_premise(name, kind):
    sg, o = G.make(name, kind), G.oracle(name, kind)
    det = _detector(sg)
    try:
        assert not det.exact_delta and det.d_etot is not None  # the fp32 path with its partials
        d, ed = det.plan.delta(), det.plan.ed()
        P = det.batch.frames(0, 0, det.batch.T).astype(np.float64)  # [T][N]
    finally:
        det.close()
    T = o.delta.size
    assert d.shape == ed.shape == (T,) and P.shape == (T, N)
    # the premise, against the reference's own S
    Pr = o.S.T
    rhs = G.IQ_CHAIN * U * np.sqrt(1.001 * Pr.sum(axis=1))[:, None] + 2 * U * np.sqrt(Pr)
    lhs = np.abs(np.sqrt(P) - np.sqrt(Pr))
    lhs[:, [0, 1, N - 1]] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(rhs > 0, lhs / rhs, np.where(lhs > 0, np.inf, 0.0))
    premise = float(ratio.max())
    # soundness
    fin = np.isfinite(ed)
    err = np.abs(d - o.delta)
    assert not np.isnan(ed).any() and np.all(ed > 0)
    with np.errstate(invalid="ignore"):
        slack = float(np.max(err[fin] / ed[fin])) if fin.any() else 0.0
    print(f"CERT4 {name} {kind} frames {T} finite {fin.mean():.4f} median_ed {np.median(ed):.3g} "
          f"max_err {err.max():.3g} max_err_over_ed {slack:.3g} premise {premise:.3g}")
    t, k = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert premise <= 1.0, f"per-bin model violated: ratio {premise:.3g} at frame {t} bin {k}"
    assert np.all(err[fin] <= ed[fin]), f"bound violated: max err/ed {slack:.3g} at frame {np.argmax(np.where(fin, err - ed, -1))}"
    # not vacuous
    if name in G.ALL_FINITE:
        assert fin.all(), f"ed = +inf on {np.count_nonzero(~fin)} of {T} frames: {np.flatnonzero(~fin)[:12]}"
    if name in G.TIGHT:
        assert np.median(ed) < 1e-2
    if name in ("zeros", "dc_only"):
        assert np.all(d == 0.0)


# --------------------------------------------------------------------- the refinement's bounds
@functools.lru_cache(maxsize=None)
def _oracle_at_hop(name, kind, hop):
    """(delta, band energy, noise energy) of the reference at a hop (hop 1024: the class's cached oracle)"""
    sg = G.make(name, kind)
    S = G.oracle(name, kind).S if hop == HOP else Q.spectrogram_iq_ref(sg.i, sg.q, FS, N, N - hop)[2]
    _, _, delta = Q.band_delta_iq_ref(S, FS, N, sg.band, sg.noise)
    Eb = S[G.band_rows(*G.bins(sg.band))].sum(axis=0)
    En = S[G.band_rows(*G.bins(sg.noise))].sum(axis=0)
    return delta, Eb, En


REFINE_CASES = [(n, k, "default", HOP) for n, k in G.CASES]
REFINE_CASES += [(n, k, "goertzel", HOP) for n, k in G.CASES if k == "int16"]
REFINE_CASES += [(n, "int16", "default", 1000) for n in ("carrier_far", "lowpass")]


@pytest.mark.parametrize("name,kind,step,hop", REFINE_CASES, ids=[f"{n}-{k}-{s}-hop{h}" for n, k, s, h in REFINE_CASES])
def test_refinement_bound(name, kind, step, hop):
    """float32 input: the float64 Goertzel rows; int16: the int8 MFMA step, or the Goertzel one with
    MSD_OPT_REFINE_GOERTZEL; hop 1000: the direct one-lane-per-block step"""
    sg = G.make(name, kind)
    ref, Eb, En = _oracle_at_hop(name, kind, hop)
    ctx = _lib.Context(0)
    try:
        ctx.set_option(_lib.OPT_REFINE_GOERTZEL, 1 if step == "goertzel" else 0)
        det = _detector(sg, ctx, hop)
        try:
            T, path = det.T, det.delta_path
            det._refine_local([(0, 100), (250, T)])
            d, ed = det.plan.delta(), det.plan.ed()
        finally:
            det.close()
    finally:
        ctx.close()
    assert T == ref.size
    sel = np.r_[0:100, 250:T]
    err = np.abs(d[sel] - ref[sel])
    e = ed[sel]
    fin = np.isfinite(e)
    with np.errstate(invalid="ignore", divide="ignore"):
        slack = float(np.max(err[fin] / e[fin])) if fin.any() else 0.0
    print(f"CERT5 {name} {kind} {step} hop {hop} path {path} frames {sel.size} finite {fin.mean():.4f} "
          f"max_ed {e[fin].max() if fin.any() else np.inf:.3g} median_ed {np.median(e):.3g} max_err {err.max():.3g} "
          f"max_err_over_ed {slack:.3g}")
    assert not np.isnan(e).any() and np.all(e > 0)
    assert np.all(err[fin] <= e[fin]), f"refined bound violated: max err/ed {slack:.3g}"
    live = (Eb[sel] > 0) & (En[sel] > 0)
    assert np.all(fin[live]), f"refined ed = +inf on {np.count_nonzero(live & ~fin)} frames with energy in both bands"
    if kind == "int16" and hop == HOP and step == "default" and name not in ("dc_band_2_4", "nyquist"):
        assert path == _lib.REFINE_INT8_MFMA
    if hop == 1000:
        assert path == _lib.REFINE_DIRECT


# ------------------------------------------------------------ end to end: what "certified" means
def _end_state(r):
    states = (bool(r.certified), bool(r.near_tie), bool(r.refine_budget_exhausted))
    assert sum(states) == 1, f"certified / near_tie / refine_budget_exhausted = {states}"
    assert 1 <= r.detector_passes <= CertifyingShard.MAX_REFINE + 1
    return ("certified", "near_tie", "exhausted")[states.index(True)]


def _same_detections(dets, rdets):
    assert [(d.t_start, d.t_stop) for d in dets] == [(x[0], x[1]) for x in rdets]
    for d, x in zip(dets, rdets):
        assert abs(d.dB - x[3]) < 1e-9, (d.dB, x[3])


@pytest.mark.parametrize("delta", ["fp32", "auto"])
@CASES
def test_end_to_end(name, kind, delta):
    sg, o = G.make(name, kind), G.oracle(name, kind)
    dets, _, dl, r = iq.proc_iq_samples(sg.i, sg.q, FS, sg.band, sg.noise, delta=delta, **KW)
    state = _end_state(r)
    print(f"CERT6 {name} {kind} {delta} {state} passes {r.detector_passes} refined {r.refined_delta_frames} of {o.delta.size} "
          f"uncertain_initial {r.uncertain_initial} detections {len(dets)} oracle {len(o.dets)}")
    if state == "certified":
        _same_detections(dets, o.dets)
    if np.all(o.delta[1:] == o.thr[1:]):  # delta equals its threshold at every decision: never certified
        assert name in ("zeros", "dc_only")
        assert len(dets) == 0 and r.certified is False and r.near_tie is True
    elif name in ("zeros", "dc_only"):
        raise AssertionError("the oracle no longer ties on a constant stream")
    if sg.pings:
        assert state == "certified" and len(dets) >= 1


@pytest.mark.parametrize("name", ["white", "dropout"])
def test_end_to_end_global_threshold(name):
    """the global detector (main.py:404-412): its threshold reads every frame of the stream"""
    sg, o = G.make(name, "int16"), G.oracle(name, "int16")
    rdets, _ = O.get_detections_ref(o.delta, 4.0, HOP / FS, None)
    for delta in ("fp32", "auto"):
        dets, _, _, r = iq.proc_iq_samples(sg.i, sg.q, FS, sg.band, sg.noise, delta=delta,
                                           flag_adaptive_threshold=False)
        state = _end_state(r)
        print(f"CERT6 {name} int16 {delta} global {state} passes {r.detector_passes} refined {r.refined_delta_frames} "
              f"detections {len(dets)} oracle {len(rdets)}")
        assert state == "certified"
        _same_detections(dets, rdets)
