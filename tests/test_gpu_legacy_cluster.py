"""GPU: the spectrogram-fed burst clustering end to end (meteorgpu.legacy.detect_and_cluster_bursts_spec):
specgram and vmin on the device -> cells above the floor -> DBSCAN, boxes, critical rule, against
tests/cluster_ref.py run on the GPU's own downloaded spectrogram and vmin."""
import numpy as np
import pytest

import cluster_ref as R

pytestmark = pytest.mark.gpu

FS = 5000
# two echoes at different Doppler offsets that overlap in time, one sub-0.2 s ping, and one speck: a tone at a bin
# centre (bin 350) lasting exactly frame 25, 2.7 dB above the floor at its peak cell and below it everywhere else
TONES = [(8.0, 3.0, 900.0, 1500.0), (9.0, 3.0, 1100.0, 1500.0), (20.0, 0.15, 1000.0, 4000.0),
         (25 * 1024 / FS, 2048 / FS, 350 * FS / 2048, 200.0)]


@pytest.fixture(scope="module")
def scene():
    from meteorgpu import legacy, synth
    x = synth.synth_tones(77, FS, 30.0, TONES)
    out, info = legacy.detect_and_cluster_bursts_spec(x, FS, details=True)
    return x, out, info


def test_output_equals_the_restatement_on_the_gpus_own_spectrogram(scene):
    from meteorgpu import legacy
    x, out, info = scene
    P, f, t, vmin, _ = legacy.noise_floor(x, FS)
    assert P.shape == (1025, 145) and vmin == info["vmin"]
    rows = np.nonzero((f >= 800.0) & (f <= 1200.0))[0]
    assert (rows[0], rows[-1], rows.size) == (328, 491, 164) == (info["k_lo"], info["k_hi"], 164)
    thr = 10.0 ** (vmin / 10)
    pts, cells, ncand = R.spec_peaks(P, 145, 328, 491, thr, legacy.SPEC_SX, legacy.SPEC_SY, 500)
    assert ncand == info["ncand"] and np.array_equal(cells, info["cells"])
    assert pts.tobytes() == info["points"].tobytes()
    lab, boxes, crit, summ = R.cluster(pts, 30.0, 5, 5.0)
    assert np.array_equal(lab, info["labels"])
    bursts, unique_labels, positions, critical, non_critical = out
    assert unique_labels == set(int(v) for v in lab)
    assert positions == [tuple(b) for b in boxes] and bursts == positions
    assert critical == list(np.nonzero(crit)[0]) and non_critical == list(np.nonzero(~crit)[0])
    # every point lies on the reference image: 496 x 366 px
    assert pts[:, 0].max() < 496 and pts[:, 1].max() < 366 and pts.min() >= 0


def test_the_scene_is_read_as_built(scene):
    from meteorgpu import legacy
    _, out, info = scene
    _, unique_labels, positions, critical, non_critical = out
    lab, pts = info["labels"], info["points"]
    nk = 164

    def cluster_at(t_s, f_hz):
        """the label of the cell at time t_s, frequency f_hz"""
        t = int(round((t_s * FS - 1024) / 1024))
        k = int(round(f_hz * 2048 / FS)) - 328
        i = np.nonzero(info["cells"] == t * nk + k)[0]
        assert i.size == 1, (t_s, f_hz)
        return int(lab[i[0]])

    a, b, ping = cluster_at(9.5, 900.0), cluster_at(10.5, 1100.0), cluster_at(20.1, 1000.0)
    assert len({a, b, ping}) == 3 and min(a, b, ping) >= 0  # the simultaneous echoes are separate clusters
    assert positions[a][2] > positions[b][0] and positions[b][2] > positions[a][0]  # ... that overlap in time
    assert a in critical and b in critical
    assert positions[ping][2] - positions[ping][0] < 5.0 and ping in non_critical  # under 0.2 s: 2 frames, 3.4 px
    assert cluster_at(25 * 1024 / FS + 0.2048, 350 * FS / 2048) == -1 and -1 in unique_labels  # the speck is noise
    assert (lab == -1).sum() == 1 and len(positions) == 3
    assert legacy.SPEC_SX == 496 / 145 and legacy.SPEC_SY == 366 / 164


def test_batched_form_equals_per_segment(scene):
    from meteorgpu import legacy, synth
    x, out, _ = scene
    segs = [x, synth.synth_tones(78, FS, 30.0, TONES[:2]), synth.synth_tones(79, FS, 30.0, []), x[::-1].copy(), x]
    single = [legacy.detect_and_cluster_bursts_spec(s, FS) for s in segs]
    assert single[0] == out and single[4] == out
    assert legacy.detect_and_cluster_bursts_spec_batch(segs, FS) == single
    assert legacy.detect_and_cluster_bursts_spec_batch(segs, FS, batch=2) == single
    assert len(single[1][2]) == 2 and single[2][2] == [] and single[2][1] == set()
    # the 5-tuples feed the hourly CSV (prime_detection.py:229-245)
    assert [(len(r[3]), len(r[4])) for r in single[:3]] == [(2, 1), (2, 0), (0, 0)]


def test_audio_shim_is_unchanged(scene):
    from meteorgpu import legacy
    from oracle import dsp_oracle as O
    x, _, _ = scene
    bursts, labels, pos, crit, noncrit = legacy.detect_and_cluster_bursts_audio(x, FS)
    ref, *_ = O.proc_samples_ref(x, FS, 0.1, (950.0, 1050.0), (650.0, 750.0), 1024, 4.0)
    assert [(d.t_start, d.t_stop) for d in bursts] == [(r[0], r[1]) for r in ref]
    assert labels == set(range(len(bursts))) and pos == [(d.t_start, d.t_stop) for d in bursts]
    assert crit == [i for i, d in enumerate(bursts) if d.dur_s >= 0.5]
    assert noncrit == [i for i, d in enumerate(bursts) if d.dur_s < 0.5]
