"""CPU: pins tests/echo_ref.py, the numpy restatement the GPU tests hold the echo kernel to -- hand-made 5 x 8
spectrograms with known answers, the span rules, and one physical case: a decaying, drifting tone in noise
through scipy.signal.spectrogram, whose frequency and e-fold time the measurement must recover."""
import numpy as np
import pytest

import echo_ref as R


def _grid(cells):
    v = np.zeros((5, 8))
    for (k, t), x in cells.items():
        v[k, t] = x
    return v


def _one(v, band, noise=(0, -1), det=(0, 8)):
    """blocks of one sample, nperseg 1, hop 1: frame t is sample t, the span of (0, 8) is all 8 frames"""
    dets = np.array([(det[0], det[1], 0.0)], R.DET_DTYPE)
    rec, _ = R.measure(v, v.shape[1], dets, R.cfg(1, 1, 1, band, noise))
    return rec[0]


def test_single_hot_cell():
    e = _one(_grid({(2, 3): 7.0, (4, 3): 2.0}), (1, 3), (4, 4))
    assert (e["t0"], e["t1"], e["t_peak"], e["k_peak"], e["p_peak"], e["n_peak"]) == (0, 8, 3, 2, 7.0, 2.0)
    assert (e["d_peak"], e["t_half_first"], e["t_half_last"], e["t_efold"], e["flags"]) == (0.0, 3, 3, 4, 0)
    assert [e[n] for n in R.SUMS] == [7.0, 2.0, 7.0, 21.0, 63.0, 21.0]


def test_two_frame_tie_lowest_frame_wins():
    e = _one(_grid({(2, 2): 5.0, (2, 6): 5.0, (2, 7): 4.0}), (2, 2))
    assert (e["t_peak"], e["t_half_first"], e["t_half_last"], e["t_efold"], e["flags"]) == (2, 2, 7, 3, 0)


def test_two_row_tie_lowest_row_wins():
    e = _one(_grid({(1, 4): 3.0, (3, 4): 3.0}), (1, 3))
    assert (e["t_peak"], e["k_peak"], e["p_peak"], e["w_r"]) == (4, 1, 6.0, 0.0)


def test_peak_in_edge_rows_has_no_parabola():
    e = _one(_grid({(0, 1): 4.0, (1, 1): 3.0}), (0, 1))
    assert (e["k_peak"], e["d_peak"], e["p_peak"]) == (0, 0.0, 7.0)
    e = _one(_grid({(4, 1): 4.0, (3, 1): 3.0}), (3, 4))
    assert (e["k_peak"], e["d_peak"], e["w_r"]) == (4, 0.0, 7.0)


def test_parabola():
    e = _one(_grid({(1, 5): 2.0, (2, 5): 4.0, (3, 5): 2.0}), (2, 2))
    assert (e["k_peak"], e["d_peak"]) == (2, 0.0)
    v = _grid({(1, 5): 1.0, (2, 5): 4.0, (3, 5): 3.0})  # a, b, c = 1, 4, 3
    e = _one(v, (2, 2))  # the neighbours lie outside the band
    assert (e["k_peak"], e["d_peak"], e["p_peak"], e["w_r"]) == (2, 0.25, 4.0, 1.0)
    e = _one(v, (1, 3))
    assert (e["k_peak"], e["d_peak"], e["p_peak"], e["w_r"]) == (2, 0.25, 8.0, 10.0)
    e = _one(_grid({(1, 5): 4.0, (2, 5): 4.0, (3, 5): 4.0}), (2, 2))  # flat: den = 0, no offset
    assert e["d_peak"] == 0.0


def test_peak_in_last_frame_and_empty_span():
    v = _grid({(2, 7): 1.0})
    e = _one(v, (2, 2))
    assert (e["t_peak"], e["t_efold"], e["flags"]) == (7, 8, 4 | 8)
    e = _one(v, (2, 2), det=(9, 9))
    assert (e["t0"], e["t1"], e["t_peak"], e["t_half_first"], e["t_half_last"], e["t_efold"]) == (8,) * 6
    assert (e["k_peak"], e["flags"], e["d_peak"]) == (-1, 0, 0.0) and np.isnan(e["p_peak"]) and np.isnan(e["n_peak"])
    assert all(e[n] == 0.0 for n in R.SUMS)
    assert e["p_peak"].tobytes() == np.float64(np.nan).tobytes()


def test_cells_are_converted_once_and_summed_in_ascending_k():
    v = np.zeros((5, 8), np.float32)
    v[0:3, 2] = [2.0 ** 24, 1.0, 1.0]  # float32 would lose both ones; float64 keeps them
    e = _one(v, (0, 2))
    assert e["p_peak"] == 2.0 ** 24 + 2.0
    w = np.zeros((5, 8))
    w[0:3, 2] = [1.0, 2.0 ** 53, -2.0 ** 53]  # ascending k: (1 + 2^53) - 2^53 = 0, any other order gives 1
    assert _one(w, (0, 2))["p_peak"] == 0.0


def test_span_rules():
    assert [R.first_frame_at(s, 1024, 128) for s in (-5, 0, 511, 512, 513, 640, 641)] == [0, 0, 0, 0, 1, 1, 2]
    c = R.cfg(100, 8, 10, (0, 0), pre=5, post=30)  # c(100 b) = 10 b
    d = np.array([(2, 4, 0.0), (4, 5, 0.0), (9, 9, 0.0)], R.DET_DTYPE)
    assert R.span(d, 0, c, 200) == (20, 40, 15, 40)   # the neighbour touches: no post padding
    assert R.span(d, 1, c, 200) == (40, 50, 40, 80)
    assert R.span(d, 2, c, 200) == (90, 90, 85, 120)  # start == stop: the padding alone
    assert R.span(d, 2, c, 100) == (90, 90, 85, 100)  # clipped at T
    assert R.span(d, 1, c, 0) == (0, 0, 0, 0)
    assert R.span(d[:1], 0, R.cfg(100, 8, 10, (0, 0), pre=50), 200) == (20, 40, 0, 40)
    rec, _ = R.measure(np.ones((1, 200)), 200, d, c)
    assert list(rec["flags"] & 3) == [2, 1, 0]


@pytest.fixture(scope="module")
def tone():
    from scipy.signal import spectrogram
    fs, n = 6000, 6000 * 5
    rng = np.random.default_rng(20240611)
    t = np.arange(n) / fs
    on = t >= 2.0
    tau, f0, drift = 0.4, 1003.3, 4.0
    phase = 2 * np.pi * (f0 * (t - 2.0) + 0.5 * drift * (t - 2.0) ** 2)
    x = rng.normal(0.0, 1.0, n) + np.where(on, 40.0 * np.exp(-(t - 2.0) / tau) * np.sin(phase), 0.0)
    _, _, S = spectrogram(x, fs, window="hann", nperseg=1024, noverlap=1024 - 128)
    dets = np.array([(10, 13, 0.0)], R.DET_DTYPE)  # blocks of 1200 samples: 2.0 s .. 2.6 s
    c = R.cfg(1200, 1024, 128, (169, 173), (118, 121), pre=4, post=46)
    rec, _ = R.measure(S, S.shape[1], dets, c)
    return rec[0], fs, tau, f0, drift


def test_physical_tone_frequency_and_decay(tone):
    e, fs, tau, f0, _ = tone
    f_peak = (e["k_peak"] + e["d_peak"]) * fs / 1024
    print(f"f_peak {f_peak:.3f} Hz (tone {f0}); e-fold {e['t_efold'] - e['t_peak']} frames "
          f"(tau / 2 = {tau / 2 * fs / 128:.2f})")
    assert abs(f_peak - f0) < 0.5 * fs / 1024  # half a bin, 2.93 Hz
    assert abs((e["t_efold"] - e["t_peak"]) - tau / 2 * fs / 128) <= 2.0  # power decays with tau / 2
    assert e["flags"] & 4 == 0 and 169 <= e["k_peak"] <= 173


def test_parameters_are_the_same_code_for_any_records(tone):
    from meteorgpu import echo
    e, fs, tau, f0, drift = tone
    p = echo.parameters(np.array([e]), fs, 1024, 128, 1024, (169, 173), (118, 121))[0]
    assert p["f_peak_hz"] == (e["k_peak"] + e["d_peak"]) * fs / 1024
    assert p["t_peak_s"] == (512 + e["t_peak"] * 128) / fs and abs(p["t_peak_s"] - 2.0) < 0.15
    assert p["peak_db"] == 10 * np.log10(e["p_peak"]) and p["energy"] == e["e_sig"] and p["flags"] == e["flags"]
    assert abs(p["efold_s"] - tau / 2) <= 2 * 128 / fs and p["snr_db"] > 10
    assert abs(p["f_mean_hz"] - f0) < fs / 1024 and np.isfinite(p["drift_hz_per_s"])
    assert p["dur_3db_s"] == (e["t_half_last"] - e["t_half_first"] + 1) * 128 / fs
    assert p["rise_s"] == (e["t_peak"] - e["t_half_first"]) * 128 / fs
    empty = np.zeros(1, echo.ECHO_DTYPE)
    empty["p_peak"], empty["k_peak"], empty["flags"] = np.nan, -1, 3
    q = echo.parameters(empty, fs, 1024, 128, 1024, (169, 173))[0]
    assert all(np.isnan(q[n]) for n in echo.PARAM_FIELDS if n not in ("energy", "flags", "t_peak_s"))
