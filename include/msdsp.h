/*
 * msdsp.h — C-ABI of libmsdsp.so, the MI355X (gfx950) implementation of the
 * meteor-scatter DSP hot path:
 *
 *   samples ──► STFT power spectrogram (scipy.signal.spectrogram semantics)
 *           └─► block framing → symmetric Hann → rFFT crop → band / noise dB → delta
 *               └─► global / adaptive threshold detector → detections (+ per-hour counts)
 *
 * The reference (th-nuernberg/meteor-scatter) is pure Python; its "FFI" for this
 * path is the numpy/scipy calls inside dsp/src/main.py.  Each entry point below
 * names the reference lines it replaces.  Conventions:
 *   - every function returns MSD_OK (0) or a negative MSD_ERR_* code; the message
 *     of the last failure on the calling thread is in msd_last_error();
 *   - "_dev" functions take device pointers and enqueue on the context's stream
 *     (no host synchronisation); the others take host pointers, borrow them for
 *     the duration of the call only, and return after the results are on the host;
 *   - a context is bound to one device and one HIP stream; it is not thread-safe.
 * No torch, numpy or HIP types appear in the signatures.
 */
#ifndef MSDSP_H
#define MSDSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSD_ABI_VERSION 1

#define MSD_OK 0
#define MSD_ERR_INVALID (-1)     /* bad argument (null pointer, size, ...)                 */
#define MSD_ERR_HIP (-2)         /* HIP runtime failure                                    */
#define MSD_ERR_UNSUPPORTED (-3) /* configuration outside what the kernels implement       */
#define MSD_ERR_ASSERT (-4)      /* a reference `assert` would fire (message says which)   */
#define MSD_ERR_CAPACITY (-5)    /* output capacity too small                              */
#define MSD_ERR_INDEX (-6)       /* reference would raise IndexError (empty global input)  */
#define MSD_ERR_RCCL (-7)        /* RCCL missing or failed                                 */

/* sample formats, as scipy.io.wavfile.read returns them (io/wavfile.py:568-733) */
#define MSD_U8 1
#define MSD_I16 2
#define MSD_I32 3
#define MSD_F32 4
#define MSD_F64 5
/* complex (I/Q) samples, interleaved I, Q: one complex sample = 2 elements */
#define MSD_CI16 6
#define MSD_CF32 7

typedef struct msd_ctx msd_ctx;
typedef struct msd_stft_plan msd_stft_plan;
typedef struct msd_block_plan msd_block_plan;
typedef struct msd_comm msd_comm;

/* ---------------------------------------------------------------- context */
int msd_abi_version(void);
const char *msd_last_error(void);
int msd_device_count(int *count);
int msd_create(int device, msd_ctx **out);
void msd_destroy(msd_ctx *ctx);
int msd_synchronize(msd_ctx *ctx);

/* device memory owned by the caller, allocated through the context's device */
int msd_dev_alloc(msd_ctx *ctx, size_t bytes, void **dptr);
int msd_dev_free(msd_ctx *ctx, void *dptr);
int msd_memcpy_h2d(msd_ctx *ctx, void *dst, const void *src, size_t bytes);
int msd_memcpy_d2h(msd_ctx *ctx, void *dst, const void *src, size_t bytes);
int msd_memset_dev(msd_ctx *ctx, void *dst, int value, size_t bytes);

/* Options: MSD_OPT_GENERIC_STFT = 1 → use the generic STFT kernel even where a
 * specialised one exists (A/B testing of the kernels; results must agree).
 * MSD_OPT_GENERIC_CSTFT = 1 → the I/Q spectrogram (msd_cstft_psd*) runs the generic kernel at nperseg =
 * nfft = 4096 too, where the specialised one runs by default (A/B and tests; both within the per-bin
 * bound, not bit-identical; msd_iq_band_delta_bound_dev then takes the larger of the two chains).
 * MSD_OPT_FRESH_ALL = 1 → the C5 stream detector computes every adaptive threshold exactly up
 * front instead of only where a scan reads it (A/B of that scheme; results must agree).
 * MSD_OPT_REFINE_GOERTZEL = 1 → msd_iq_delta64_dev computes int16 blocks with the float64
 * Goertzel kernel instead of the exact int8-MFMA one (A/B; both within their bounds).
 * MSD_OPT_CSTFT_RESERVE = n → the persistent C5 spectrogram kernel (msd_cstft_psd_dev) leaves n
 * of its resident workgroup slots free, so that small kernels on another context's stream (the
 * stream detector, when its delta does not come from the spectrogram) run beside it.
 * MSD_OPT_STREAM_CUS = n → the context's stream is re-created on a subset of the device's CUs
 * (hipExtStreamCreateWithCUMask): n > 0 the first n CUs, n < 0 all but those |n| -- two contexts
 * set to n and -n split the chip into disjoint parts --, 0 all CUs again; persistent grids are
 * sized for the CUs the stream may use.  Synchronises the context's stream first.
 * MSD_OPT_CSTFT_SCHED = 0 / 1 / 2 → how the persistent C5 spectrogram kernel (hop 1024) splits the
 * frames over its workgroups: 0 (default) and 2 chunks drawn from a guided schedule by an atomic
 * ticket; 1 one fixed range per workgroup (round-4 behaviour, A/B).  Same output either way.
 * MSD_OPT_STFT_SCHED = 0 / 1 / 2 → the same choice for stft1024_kernel's 32-frame tiles (the C3
 * spectrogram): 0 (default) and 1 fixed ranges, 2 chunks.
 * MSD_OPT_BLOCK_GOERTZEL = 1 → msd_block_delta[_dev] computes int16 blocks with the float64
 * Goertzel kernel instead of the exact int8-MFMA one (plans with min(block_size, n_fft) = 256,
 * 512 or 1024 and at most 8 band + noise bins take the latter by default; A/B, both within the
 * near-tie bound of meteorgpu/margin.py).
 * MSD_OPT_WELCH_GOERTZEL = 1 → msd_welch_bands[_dev] / msd_welch_psd compute int16 samples with the
 * float64 Goertzel kernel instead of the exact int8-MFMA one (plans with nperseg 64, 128, 192, 256
 * or 512, <= 16 segments per block and a window in [-1, 1] take the latter by default; A/B,
 * both within margin.py's live bound).
 *
 * Test hooks (per context; results must agree with the default):
 * MSD_OPT_WELCH_I8_FORM = 0..3 → which form of the int8-MFMA Welch kernel a launch takes.  Bit 0:
 * the eight-term float64 digit sum even where the plan's bound allows int32 pairs.  Bit 1: the
 * generic instantiation even for the live default's shape (nperseg 256, 5 segments per block).
 * Read at launch, so it takes effect on existing plans.  Every form gives bit-identical output.
 * MSD_OPT_STREAM_EPS_LOG2 = n in 0..1023 → the C5 stream detector's near-tie bound is widened by
 * 2^n (never narrower than the bound), so more frames are made exact; same decisions. */
#define MSD_OPT_GENERIC_STFT 1
#define MSD_OPT_FRESH_ALL 2
#define MSD_OPT_REFINE_GOERTZEL 3
#define MSD_OPT_CSTFT_RESERVE 4
#define MSD_OPT_STREAM_CUS 5
#define MSD_OPT_CSTFT_SCHED 6
#define MSD_OPT_STFT_SCHED 7
#define MSD_OPT_BLOCK_GOERTZEL 8
#define MSD_OPT_WELCH_GOERTZEL 9
#define MSD_OPT_WELCH_I8_FORM 10
#define MSD_OPT_STREAM_EPS_LOG2 11
#define MSD_OPT_GENERIC_CSTFT 12
int msd_set_option(msd_ctx *ctx, int option, int value);

/* Per-kernel device timing with HIP events on the context stream.
 * kernel id: 0 = STFT power, 1 = block delta, 2 = detector stats, 3 = detector scan,
 * 4 = Welch band powers, 5 = live detector, 6 = complex (I/Q) STFT, 7 = I/Q band delta,
 * 8 = stream fresh thresholds, 9 = stream scan, 10 = float64 delta (msd_iq_delta64_dev),
 * 11 = the I/Q STFT's post-FFT detrend of bins 0, +-1 (its separate fix-up kernels),
 * 12 = Welch spectrum (msd_welch_spectrum*), 13 = DDC (the down-converter's tile kernel, msd_ddc_*),
 * 14 = resampler (the rational resampler's tile kernel, msd_resamp_*),
 * 15 = burst clustering (the point extraction and the DBSCAN kernel, msd_spec_peaks_* / msd_cluster*),
 * 16 = echo measurement (msd_echo_measure*). */
int msd_timing_enable(msd_ctx *ctx, int enable);
/* which kernels get events while timing is on: bit k = kernel id k (default all); a timed
 * region that times only its roofline kernel carries no events around the others */
int msd_timing_select(msd_ctx *ctx, uint32_t kernel_mask);
int msd_timing_reset(msd_ctx *ctx);
int msd_timing_get(msd_ctx *ctx, int kernel, double *total_ms, int64_t *launches);

/* ------------------------------------------------- a7: STFT power spectrogram
 * Replaces scipy.signal.spectrogram(x, fs, window='hann', nperseg=N,
 * noverlap=N-hop, nfft=N, detrend='constant', scaling='density', mode='psd')
 * as called at dsp/src/main.py:52-54 and :132-133.
 * window: N float32 values of the periodic Hann (scipy get_window, cast to
 * complex64 by _spectral_helper, i.e. float32); scale = 1/(fs*sum(w^2)) as
 * scipy computes it.  Output: float32 [K = N/2+1][T], T = (n-N)/hop + 1, with
 * bins 1..N/2-1 doubled (one-sided, even N).  N: a power of two in [16, 16384]
 * (1024: stft1024.hip; 256..2048: stft.hip's tiled kernel; others: stft_any.hip). */
int msd_stft_plan_create(msd_ctx *ctx, int32_t nperseg, int32_t hop, const float *window, double scale,
                         msd_stft_plan **out);
/* The general form: segments of nperseg samples (any length >= 1) zero-padded to an nfft-point
 * transform (nfft a power of two in [16, 16384], nfft >= nperseg), K = nfft/2 + 1 bins, in
 * float32 (precision MSD_F32, output float) or float64 (MSD_F64, output double; the
 * msd_stft_psd_f64 entry points).  Covers scipy.signal.spectrogram(..., nfft=) and its
 * shrinking of nperseg to a short input (dsp/src/main.py:127-133 with n_fft = 1024*4,
 * :278-300; scipy _spectral_py.py _triage_segments) and matplotlib.mlab.specgram in float64
 * (prime_detection.py:70, window_hanning, detrend_none, pad_to = NFFT).  window: nperseg
 * float64 values (cast to float32 by a float32 plan). */
int msd_stft_plan_create_ex(msd_ctx *ctx, int32_t nperseg, int32_t nfft, int32_t hop, const double *window,
                            double scale, int precision, msd_stft_plan **out);
void msd_stft_plan_destroy(msd_stft_plan *plan);
/* K = nfft/2 + 1, the rows of the plan's spectrogram */
int32_t msd_stft_bins(const msd_stft_plan *plan);
/* detrend: 1 = 'constant' (scipy's default, the plan's initial setting), 0 = none
 * (matplotlib.mlab.specgram's detrend_none, prime_detection.py:70) */
int msd_stft_plan_set_detrend(msd_stft_plan *plan, int detrend);
/* frames of an n-sample signal (0 if n < nperseg) */
int64_t msd_stft_frames(const msd_stft_plan *plan, int64_t n);
/* batch, device-resident: file f occupies x[off[f] .. off[f]+len[f]) (elements of dtype);
 * its spectrogram is out[f*K*ld + k*ld + t] (ld >= max T, ld % 32 == 0; columns in
 * [T_f, ld) are written with zeros). off/len are DEVICE arrays of nfiles int64. */
int msd_stft_psd_dev(msd_stft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                     int64_t nfiles, int64_t max_frames, float *out, int64_t ld);
/* single signal, host buffers: out is dense float32 [K][T] */
int msd_stft_psd(msd_stft_plan *plan, const void *x, int dtype, int64_t n, float *out, int64_t *frames);
/* the same two for a float64 plan (msd_stft_plan_create_ex with MSD_F64): out is double */
int msd_stft_psd_f64_dev(msd_stft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                         int64_t nfiles, int64_t max_frames, double *out, int64_t ld);
int msd_stft_psd_f64(msd_stft_plan *plan, const void *x, int dtype, int64_t n, double *out, int64_t *frames);

/* --------------------------------------- a2/a3: block band energies → delta
 * Replaces the per-block loop of dsp/src/main.py:352-393:
 *   fft_block = np.fft.rfft(block * np.hanning(B), n=Nf); P = |fft_block|^2
 *   band_dB = 10*log10(sum(P[band]) + 1e-12); noise_dB likewise; delta = band_dB - noise_dB
 * block_size B = int(fs*block_duration_sec); nfft Nf (already doubled, main.py:353);
 * window: the first min(B, Nf) values of np.hanning(B) (float64);
 * band/noise: inclusive bin ranges [lo, hi] of rfftfreq(Nf, 1/fs) selected by the
 * reference masks (hi < lo means an empty band → energy 1e-12). Arithmetic is float64.
 * L = min(B, Nf) <= 65536 (above: MSD_ERR_UNSUPPORTED), at most 4096 bins in the two bands
 * together.  Three float64 kernels serve a plan (block_delta.hip): up to L = 4096 a 16-lane
 * Goertzel per block for up to 64 bins and a rotation recurrence, one wave per block, above
 * that; for 4096 < L <= 65536 a 256-lane Goertzel, one workgroup per block, for any bin count.
 * int16 blocks of L = 256, 512 or 1024 with 1-8 bins run on the matrix cores (block_i8.hip). */
int msd_block_plan_create(msd_ctx *ctx, int64_t block_size, int32_t nfft, const double *window, int32_t band_lo,
                          int32_t band_hi, int32_t noise_lo, int32_t noise_hi, msd_block_plan **out);
void msd_block_plan_destroy(msd_block_plan *plan);
/* batch, device-resident; block count of file f = len[f] / B; outputs [nfiles][ld]
 * (band_db / noise_db may be NULL) */
int msd_block_delta_dev(msd_block_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                        int64_t nfiles, int64_t max_blocks, double *band_db, double *noise_db, double *delta,
                        int64_t ld);
int msd_block_delta(msd_block_plan *plan, const void *x, int dtype, int64_t n, double *band_db, double *noise_db,
                    double *delta, int64_t *blocks);

/* ------------------------------------------------- a4/a5: threshold detector
 * adaptive = 0: get_detections()          dsp/src/main.py:396-448
 * adaptive = 1: get_detections_adaptive() dsp/src/main.py:450-522
 * Block counts are the host's int(x_sec / block_duration_sec) (main.py:458-461).
 * mean/std follow numpy (pairwise summation, population std) in float64 without
 * FMA contraction.  A detection is the block range [start, stop) and the mean of
 * delta over it (the reference's db_mean). */
typedef struct {
    int32_t adaptive;
    int32_t reserved;
    double k_std;                 /* threshold_std_factor              */
    int64_t window_blocks;        /* int(threshold_estimation_window_sec / bs)         */
    int64_t freeze_before_blocks; /* int(threshold_freeze_before_detection_sec / bs)   */
    int64_t freeze_after_blocks;  /* int(threshold_freeze_after_detection_sec / bs)    */
    int64_t fixed_init_blocks;    /* int(threshold_fixed_init_duration_sec / bs)       */
} msd_det_cfg;

typedef struct {
    int64_t start; /* first block                           */
    int64_t stop;  /* one past the last block (t_stop/bs)   */
    double db;     /* np.mean(delta[start:stop])            */
} msd_det;

/* optional per-hour histogram of detection starts (main.py:687-696 Counter of
 * utc_start.replace(minute=0, ...)): bucket = floor((file_start_us[f] +
 * round(start*block_sec*1e6) - base_us) / bucket_us); outside [0, nbuckets) → dropped */
typedef struct {
    const int64_t *file_start_us; /* device, nfiles  */
    int64_t base_us;
    int64_t bucket_us;
    int32_t nbuckets;
    int32_t reserved;
    double block_sec;
    int64_t *counts; /* device, nbuckets, accumulated (not cleared) */
} msd_hist_cfg;

/* status word per file (device int32): 0 ok, 1 zero-duration global detection (reference
 * assert at main.py:437), 2 empty global input (IndexError at main.py:412), 3 capacity
 *
 * Held bit for bit to the float64 numpy restatement of the reference over every file of a launch,
 * whatever the other files are (tests/test_gpu_detect_contract.py):
 *   - margin[f] is the minimum over all nblocks[f] blocks of |delta - threshold used| (adaptive:
 *     the thresholds list's entry of that block; global: the single threshold), NaN terms
 *     ignored, +inf if no term is left (no blocks, or a NaN threshold everywhere);
 *   - delta columns at or past nblocks[f] are not read; thresholds is written at [0, nblocks[f])
 *     of the row (global mode: entry 0 alone, NaN for an empty file);
 *   - status 3 (more detections than cap): counts[f] is the full count and the first cap entries
 *     are complete (start, stop, db); the histogram counts the stored detections only, i.e. the
 *     first cap of that file.  Files within cap are unaffected;
 *   - status 1 and 2 concern their own file only.  On status 1 the zero-duration detection is
 *     counted and stored last (start = stop = nblocks[f] - 1, db = NaN);
 *   - a block equal to its threshold is not above it (the reference's >);
 *   - +inf, -inf and NaN blocks follow numpy's arithmetic as the reference would: a window or file
 *     that holds one has a NaN threshold and nothing in it fires, a +inf block above a finite
 *     threshold is a detection with db = +inf. */
int msd_detect_dev(msd_ctx *ctx, const double *delta, const int64_t *nblocks, int64_t nfiles, int64_t ld,
                   const msd_det_cfg *cfg, msd_det *dets, int64_t cap, int64_t *counts, double *thresholds,
                   double *margin, int32_t *status, const msd_hist_cfg *hist);
/* single file, host buffers. thresholds (nb) and margin may be NULL.
 * global mode: *thresholds receives the single threshold in thresholds[0]. */
int msd_detect(msd_ctx *ctx, const double *delta, int64_t nb, const msd_det_cfg *cfg, msd_det *dets, int64_t cap,
               int64_t *count, double *thresholds, double *margin);

/* --------------------------------------- C5: two-sided STFT of complex (I/Q) input
 * scipy.signal.spectrogram(z, fs, 'hann', nperseg, noverlap=nperseg-hop, nfft) for complex z (BASELINE
 * config C5: 192 kHz I/Q, 4096-point frames, 75 % overlap): two-sided, bins in FFT order (0..nfft/2-1,
 * -nfft/2..-1), |X|^2 * scale, no doubling, constant detrend of the complex mean of the nperseg samples
 * (before the zero padding), zeros past nperseg, complex64 arithmetic.
 * Shapes: any 1 <= nperseg <= nfft, nfft a power of two in [16, 8192], any 1 <= hop <= nperseg.  8192 is the
 * real path's limit too (stft_any at nfft 16384 = 8192 complex points): above it MSD_ERR_UNSUPPORTED.
 * nperseg = nfft = 4096 runs the kernel specialised to it, everything else the generic one
 * (MSD_OPT_GENERIC_CSTFT: that one at 4096 too).  A stream shorter than nperseg has 0 frames.
 * window: nperseg float32 (periodic Hann); scale = 1/(fs*sum(w^2)).  msd_cstft_plan_create is the
 * nfft = nperseg case of msd_cstft_plan_create_ex; msd_cstft_nfft gives a plan's row length.
 * Output FRAME-major: out[(s*max_frames + t)*nfft + k] (scipy's Sxx[k][t] transposed; a
 * frequency-major tile of 4096 rows would not fit in LDS); frames past a stream's end are 0.
 * off/len: device int64 arrays in complex samples; dtype MSD_CI16 or MSD_CF32.
 * msd_cstft_chain (host only, no context): the rounding-chain constant c of the kernel that runs the
 * shape -- every bin's amplitude is within c * 2^-24 * sqrt(sum_k out[k]) (+ 3 * 2^-24 of itself) of the
 * float64 reference's: 37 at 4096 / 4096, else the generic kernel's count of its passes
 * (csrc/cstft_chain.h). */
typedef struct msd_cstft_plan msd_cstft_plan;
int msd_cstft_plan_create(msd_ctx *ctx, int32_t nperseg, int32_t hop, const float *window, double scale,
                          msd_cstft_plan **out);
int msd_cstft_plan_create_ex(msd_ctx *ctx, int32_t nperseg, int32_t nfft, int32_t hop, const float *window,
                             double scale, msd_cstft_plan **out);
int32_t msd_cstft_nfft(const msd_cstft_plan *plan);
int msd_cstft_chain(int32_t nperseg, int32_t nfft, double *chain);
void msd_cstft_plan_destroy(msd_cstft_plan *plan);
int msd_cstft_set_detrend(msd_cstft_plan *plan, int detrend);
int64_t msd_cstft_frames(const msd_cstft_plan *plan, int64_t n);
int msd_cstft_psd_dev(msd_cstft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                      int64_t nstreams, int64_t max_frames, float *out);
/* the same, plus (etot != NULL) each frame's total power sum_k out[k] as 16 float32 partials,
 * etot[i*stride + s*max_frames + t] (device, stride = msd_cstft_energy_stride(nstreams,
 * max_frames)): Parseval's input norm for the fp32 FFT's per-bin error bound
 * (msd_iq_band_delta_bound_dev).  The partials are the frame's own (their sum is the float32 sum
 * of out[k], within 1e-4 relative: times 1.001 an upper bound); entries of frames past a stream's
 * end are not written */
int msd_cstft_psd_energy_dev(msd_cstft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                             int64_t nstreams, int64_t max_frames, float *out, float *etot);
/* the same, with each frame's complex sample sum given (frame_sums: device double [nstreams *
 * max_frames][2], (sum I, sum Q) of frame s*max_frames + t, e.g. from msd_iq_delta64_sums_dev):
 * at the C5 shape (4096 / 4096, hop 1024) the kernel then takes each frame's detrend mean from these sums
 * and computes none itself; other hops and the generic kernel ignore them.  Exact sums (int16 input) give output bit-identical to
 * msd_cstft_psd_energy_dev.  Either way the mean is subtracted before the window as an exact
 * two-part float32 value (hi + lo), so the result is scipy's within float32 rounding of the
 * detrended samples whatever the DC offset. */
int msd_cstft_psd_fsums_dev(msd_cstft_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                            int64_t nstreams, int64_t max_frames, float *out, float *etot, const double *frame_sums);
int64_t msd_cstft_energy_stride(int64_t nstreams, int64_t max_frames);
/* one stream, host buffers: n complex samples in, out float32 [T][nfft] */
int msd_cstft_psd(msd_cstft_plan *plan, const void *x, int dtype, int64_t n, float *out, int64_t *frames);

/* -------------------------------- C5: band / noise dB per frame of the I/Q spectrogram
 * The per-block band energies of dsp/src/main.py:380-393 taken per STFT frame of the two-sided
 * spectrogram (the frame is the detector's block, block_sec = hop/fs):
 *   E = sum(Sxx[mask, t]) + 1e-12;  dB = 10*log10(E);  delta = band_dB - noise_dB
 * with the masks of fftfreq(N, 1/fs) selected as (f >= lo) & (f <= hi).  Bands are inclusive
 * SIGNED bin ranges [lo, hi] in -N/2 .. N/2-1 (contiguous in frequency; bin b < 0 is column
 * b + N of the frame-major row); hi < lo = empty band (E = 1e-12).  spec: device float32
 * [s][max_frames][N] as msd_cstft_psd_dev writes it; frames: device int64 [nstreams];
 * outputs float64 [s*ld + t] (band_db / noise_db may be NULL).  Sums are float64. */
int msd_iq_band_delta_dev(msd_ctx *ctx, const float *spec, int64_t nstreams, int64_t max_frames,
                          const int64_t *frames, int32_t nperseg, int32_t band_lo, int32_t band_hi, int32_t noise_lo,
                          int32_t noise_hi, double *band_db, double *noise_db, double *delta, int64_t ld);
/* the same plus ed[s*ld + t] (device float64): a bound on |delta - delta_ref| against the float64
 * reference (scipy's spectrogram of complex128 input, its band sums and dB), from the standard
 * rounding-error model of the fp32 FFT and the frame energies etot of msd_cstft_psd_energy_dev
 * (stream.hip IQ_CHAIN; the chain is msd_cstft_chain's for rows of nperseg floats); +inf where a band
 * touches bins -1..1 (the detrend's DC term).  Rows of a zero-padded plan (nfft > nperseg) are not
 * covered: there the mean's rounding leaks past bins -1..1 (the window's transform is no longer compact
 * on the finer grid), so certification is limited to nfft = nperseg. */
int msd_iq_band_delta_bound_dev(msd_ctx *ctx, const float *spec, const float *etot, int64_t nstreams,
                                int64_t max_frames, const int64_t *frames, int32_t nperseg, int32_t band_lo,
                                int32_t band_hi, int32_t noise_lo, int32_t noise_hi, double *band_db, double *noise_db,
                                double *delta, double *ed, int64_t ld);

/* -------------------------- C5: the detector over one long stream, time-sharded over ranks
 * get_detections_adaptive() (dsp/src/main.py:450-522) and get_detections() (:396-448) over
 * the delta of ONE stream of n_total frames of which this rank holds [frame0, frame0+n_local).
 * Bit-exact with the reference's numpy arithmetic (pairwise sums in 8192-element chunks,
 * mean + k*std rounded as numpy, no FMA).  The whole-stream mean/std, the W-frame look-back
 * of the adaptive threshold and the freeze/run state at the shard edges are the only things
 * that cross ranks; the host moves them (meteorgpu/stream.py):
 *   1. halos: the tail halo holds the min(W, frame0) frames before frame0, the head halo
 *      the min(head_frames, n_total - frame0 - n_local) frames after the shard;
 *   2. msd_stream_chunk_sums: the pairwise sums of the 8192-frame chunks (of delta, or of
 *      (delta - mean)^2) that START in the shard; in chunk order, s = 0.0; s += c gives
 *      numpy's add.reduce over the whole stream;
 *   3. msd_stream_fresh + msd_stream_refine: every frame's mean + k*std(delta[max(0, i-W):i]) is
 *      state-free but only read where the detector is not frozen.  fresh() writes a cheap
 *      predictor (prefix sums; exact numpy order for windows shorter than W); each scan marks
 *      the 512-frame tiles whose fresh thresholds it read; refine() computes those tiles
 *      numpy-exactly and returns how many it computed.  Scan, refine, scan again until refine
 *      computes nothing: the last scan then read exact thresholds only;
 *   4. msd_stream_scan: the freeze/run scan of the shard from the state entering frame0,
 *      in parallel segments iterated to a fixed point; returns the state after the shard
 *      (rank r+1 enters with rank r's end state: repeat until no entry state changes);
 *   5. msd_stream_runs / msd_stream_db: the shard's runs [start, stop) (start = -1: a run
 *      continued from the previous shard) and their dB means.
 * cfg->adaptive = 0 gives the global detector (every frame uses thr0; the end quirk of
 * main.py:414-415 and the assert of :437 are the host's, on the last shard). */
typedef struct msd_stream_plan msd_stream_plan;
typedef struct {
    int64_t freeze_until; /* freeze_until_idx (main.py:455), -1 initially             */
    int64_t last_stop;    /* last frame of the last run, -2 if there is none           */
    double thr;           /* the `threshold` variable after the previous frame         */
    int64_t src;          /* the frame whose fresh threshold thr is; -1: thr0          */
    double thr_err;       /* certification: thr's error bound against the reference  */
} msd_stream_state;
int msd_stream_plan_create(msd_ctx *ctx, const msd_det_cfg *cfg, int64_t n_total, int64_t frame0, int64_t n_local,
                           int64_t seg_len, int64_t cap_per_seg, int64_t head_frames, msd_stream_plan **out);
void msd_stream_plan_destroy(msd_stream_plan *plan);
/* device pointers into the plan: the shard's delta (n_local, written by the caller, e.g. by
 * msd_iq_band_delta_dev), the tail halo (n_tail = min(W, frame0)), the head halo, and the
 * thresholds actually used per frame (after msd_stream_scan).  Any may be NULL. */
int msd_stream_buffers(msd_stream_plan *plan, double **delta, double **tail, int64_t *n_tail, double **head,
                       int64_t *n_head, double **thresholds);
/* use_mean = 0: sums of delta; 1: sums of (delta - mean)^2.  Synchronous; sums -> host
 * (cap >= chunks), *first_chunk = global index of the first chunk. */
int msd_stream_chunk_sums(msd_stream_plan *plan, int32_t use_mean, double mean, double *sums, int64_t cap,
                          int64_t *nchunks, int64_t *first_chunk);
/* on = 1 (default): every threshold the scan reads is numpy-exact, so the thresholds buffer holds
 * the reference's `thresholds` list.  on = 0 (decisions only): thresholds are predicted with a
 * rounding-error bound, and made exact only for the frames where a decision is within the bound
 * or where a detection holds the threshold; the detections are the same, the thresholds buffer
 * is not the reference's list.  Call before msd_stream_fresh. */
int msd_stream_set_exact_thresholds(msd_stream_plan *plan, int32_t on);
int msd_stream_fresh(msd_stream_plan *plan); /* async; needs the tail halo */
/* decisions-only mode, after msd_stream_fresh and before any refine: the predicted thresholds
 * and their error bounds (n_local each, host; either may be NULL) -- for checking the bound */
int msd_stream_predicted(msd_stream_plan *plan, double *fresh, double *eps);
/* synchronous; *computed = tiles (decisions only: frames) made exact now (0: the previous scan
 * read exact values only where they decide) */
int msd_stream_refine(msd_stream_plan *plan, int32_t *computed);
/* thr0 = mean + k*std of the whole stream.  reset = 1: every segment restarts from the clean
 * state (first call); 2: every segment re-scans from its last fixed-point entry state (after a
 * refine changed thresholds); 0: only the shard's entry state changed.  Synchronous; *rounds =
 * scan launches. */
int msd_stream_scan(msd_stream_plan *plan, double thr0, const msd_stream_state *entry, int32_t reset,
                    msd_stream_state *exit_state, int32_t *rounds);
/* the shard's runs in order, host out; stop is exclusive; margin = min |delta - thr| */
int msd_stream_runs(msd_stream_plan *plan, msd_det *runs, int64_t cap, int64_t *count, double *margin);
/* dets[j].db = np.mean(delta[start:stop]) for global [start, stop) inside the halos + shard */
int msd_stream_db(msd_stream_plan *plan, msd_det *dets, int64_t n);
/* One process holding the whole stream (frame0 = 0, n_local = n_total): the sequence above in
 * one call -- fresh, global threshold, scan / refine to the fixed point, runs (the global
 * mode's end quirk applied), dB means.  out: cap runs, *count of them; *thr0_out = mean +
 * k*std of the stream; *margin = min |delta - threshold read|; *rounds = scans; *refined =
 * exact-threshold work units (tiles, or frames with exact_thresholds = 0).  Errors as the
 * reference: MSD_ERR_INDEX (empty global input), MSD_ERR_ASSERT (zero-duration last run). */
int msd_stream_detect_local(msd_stream_plan *plan, int32_t exact_thresholds, msd_det *out, int64_t cap,
                            int64_t *count, double *thr0_out, double *margin, int32_t *rounds, int32_t *refined);

/* Certification against the float64 reference (C5: delta from the fp32 spectrogram).  With
 * msd_stream_set_certify(plan, 1) every scan also checks each decision delta > thr of the final
 * trajectory against error bounds: ed per frame (|delta - delta_ref|, written by
 * msd_iq_band_delta_bound_dev into msd_stream_error_buffers' local part; halos exchanged like
 * delta's; 0 = exact), the fresh thresholds' bound mean(ed) + |k| rms(ed) over their window
 * (computed by msd_stream_fresh), and thr0's over the whole stream (msd_stream_set_terr0 from the
 * ranks' msd_stream_ed_sums; msd_stream_detect_local computes it itself).  A decision with
 * |delta - thr| <= ed + threshold bound (+ the predictor's bound, decisions only) is uncertain;
 * msd_stream_certificate returns their count, the smallest slack, the largest error zone (ed +
 * threshold bound) of any decision and up to cap of them as
 * (global frame, frame whose window gave the threshold, -1 = thr0).  Zero uncertain decisions:
 * the detections are the reference's.  msd_stream_certificate fails (MSD_ERR_INVALID) unless the
 * plan's last full scan ran with certification on: msd_stream_set_certify invalidates the
 * certificate until the next msd_stream_scan with reset 1 or 2 (or msd_stream_detect_local).
 * msd_iq_delta64_dev: blocks of D = gcd(nperseg, hop) samples run as 16-lane Goertzel rows when D
 * is a multiple of 64, else one lane per block (any D). */
int msd_stream_set_certify(msd_stream_plan *plan, int32_t on);
int msd_stream_error_buffers(msd_stream_plan *plan, double **ed, double **tail, double **head);
int msd_stream_ed_sums(msd_stream_plan *plan, double *sum_ed, double *sum_ed2);
int msd_stream_set_terr0(msd_stream_plan *plan, double sum_ed, double sum_ed2);
int msd_stream_certificate(msd_stream_plan *plan, int64_t *uncertain, double *min_slack, double *max_zone,
                           int64_t *frames, int64_t *srcs, int64_t cap, int64_t *listed);
/* The refinement of uncertain decisions: delta of the frames in `ranges` ([nranges][2] host
 * int64, [first, end) frame indices, sorted and disjoint; frame t starts at complex sample t*hop
 * of x) recomputed in float64 from the samples -- the reference's quantity (scipy spectrogram of
 * complex128 input, periodic Hann, constant detrend, density; band sums in np.sum order;
 * 10*log10(E + 1e-12)) by a direct DFT of the band bins (blocks of gcd(nperseg, hop) samples, the
 * Hann window as three bin taps) -- into delta[t] and its error bound against the reference into
 * ed[t] (device float64).  x: device interleaved I/Q (MSD_CI16 or MSD_CF32), n_samples complex
 * samples.  Asynchronous on the context's stream (the ranges are copied before the call
 * returns; nperseg <= 65536). */
int msd_iq_delta64_dev(msd_ctx *ctx, const void *x, int32_t dtype, int64_t n_samples, int32_t nperseg, int64_t hop,
                       double fs, int32_t band_lo, int32_t band_hi, int32_t noise_lo, int32_t noise_hi,
                       const int64_t *ranges, int64_t nranges, double *delta, double *ed);
/* the same, plus each refined frame's complex sample sum (frame_sums[2 t], [2 t + 1]: sum I, sum Q
 * as float64 -- exact for int16 input) for msd_cstft_psd_fsums_dev.  MSD_ERR_UNSUPPORTED (nothing
 * launched) when the block step carries no sums: the int8 path with at most 8 needed bins. */
int msd_iq_delta64_sums_dev(msd_ctx *ctx, const void *x, int32_t dtype, int64_t n_samples, int32_t nperseg,
                            int64_t hop, double fs, int32_t band_lo, int32_t band_hi, int32_t noise_lo,
                            int32_t noise_hi, const int64_t *ranges, int64_t nranges, double *delta, double *ed,
                            double *frame_sums);
/* Which block step msd_iq_delta64_dev takes for a geometry (host only, no GPU): int16 input with
 * blocks of D = gcd(nperseg, hop) = 1024 samples, no band touching bin 0 and at most 10 needed
 * bins (band and noise bins +- 1) runs the EXACT integer DFT on the matrix cores (int16 samples as
 * two int8 digits, the twiddles as six balanced base-256 digits, v_mfma_i32_16x16x64_i8, float64
 * combination; bound ~120 u instead of the Goertzel's ~3 L / |sin theta| u) unless
 * MSD_OPT_REFINE_GOERTZEL is set; other D % 64 == 0 the float64 Goertzel rows; any other D one
 * lane per block.  Returns the path (> 0) or an error code. */
#define MSD_REFINE_DIRECT 1
#define MSD_REFINE_GOERTZEL_ROWS 2
#define MSD_REFINE_INT8_MFMA 3
int msd_iq_delta64_path(int32_t nperseg, int64_t hop, double fs, int32_t band_lo, int32_t band_hi, int32_t noise_lo,
                        int32_t noise_hi, int32_t dtype);
/* The rounding chain behind ed for a geometry, in its three parts, in units of u = 2^-53 (host only,
 * no context): own = the block step the geometry takes (MSD_REFINE_INT8_MFMA: the three constants
 * below, 119; MSD_REFINE_GOERTZEL_ROWS: 3 L Gmax + 12 with L = D / 16 samples per lane and Gmax =
 * min(max over the needed bins of 1 / |sin theta|, L); MSD_REFINE_DIRECT: D + 4), combine = the frame
 * step ((R + 4) for the R block rotations and sums, 8 for the mean, the Hann taps and |Y|^2),
 * reference = the float64 reference's own chain (4 log2 N + 11).  frame_kernel's bound uses their sum
 * (own + (combine + reference), all integers when nperseg is a power of two).  The function honours no
 * context: goertzel != 0 gives the figures a context with MSD_OPT_REFINE_GOERTZEL set runs int16 input
 * with (the Goertzel rows instead of the int8 step).  Any of the three pointers may be NULL, not all.
 * The int8 step's own chain is the twiddles' quantisation sqrt 2 * 2^-47 (1 + 2^-16) per unit |x| (91),
 * the six-digit Horner sum (6) and the four sub-block products summed with rounded twiddles (22). */
#define MSD_REFINE_I8_CHAIN_QUANT 91.0
#define MSD_REFINE_I8_CHAIN_HORNER 6.0
#define MSD_REFINE_I8_CHAIN_SUBBLOCK 22.0
int msd_iq_delta64_chain(int32_t nperseg, int64_t hop, double fs, int32_t band_lo, int32_t band_hi, int32_t noise_lo,
                         int32_t noise_hi, int32_t dtype, int32_t goertzel, double *own, double *combine,
                         double *reference);

/* ------------------------------------------- a10: legacy spectrogram noise floor
 * prime_detection.py:65-91: band_power = np.sum(Pxx[noise_band]) sums the spectrogram over
 * the band's bins AND all frames.  spec: device float32 [nfiles][K][ld] as msd_stft_psd_dev
 * writes it; out[f] (device) = sum over k in [lo, hi], t < frames of spec, float64. */
int msd_spec_band_sum_dev(msd_ctx *ctx, const float *spec, int64_t nfiles, int32_t K, int64_t frames, int64_t ld,
                          int32_t lo, int32_t hi, double *out);
/* the same over a float64 spectrogram (msd_stft_psd_f64_dev: the legacy specgram in mlab's
 * float64) */
int msd_spec_band_sum_f64_dev(msd_ctx *ctx, const double *spec, int64_t nfiles, int32_t K, int64_t frames,
                              int64_t ld, int32_t lo, int32_t hi, double *out);

/* ------------------------------- a11: time-frequency burst clustering of the legacy spectrogram
 * meteor_detect_class/detector_and_classification.py:7-91 takes points on the 800-1200 Hz spectrogram image
 * of a 30 s grab, clusters them with DBSCAN(eps=30, min_samples=5).fit(points).labels_ (:20-21), boxes each
 * cluster (:44-46) and calls it critical when its extent along the time axis is >= 5 px (:48-50).
 *
 * msd_spec_peaks_f64*: the points, in the place of cv2.ORB_create(nfeatures=500).detectAndCompute (:12-16;
 * ORB on a JPEG is not reproducible, the cells above the colour floor are).  spec: float64 [nimg][K][ld] as
 * msd_stft_psd_f64_dev writes it (the layout of msd_spec_band_sum_f64_dev).  For image m the candidates are
 * the cells k_lo <= k <= k_hi, t < frames with spec > thr[m] (thr = 10^(vmin/10) of prime_detection.py:86-91's
 * vmin, computed by the caller: the non-background pixels of the reference image; NaN is never a candidate,
 * +inf is).  Cell index c = t nk + (k - k_lo), nk = k_hi - k_lo + 1, frame-major.  More than max_points
 * candidates: the max_points largest by (value descending, c ascending) stay (-0.0 counts as +0.0).  Points
 * are emitted in ascending c: xy[(m max_points + i) 2 + {0, 1}] = ((double)t sx, (double)(k - k_lo) sy), one
 * rounded multiply each; cell[m max_points + i] = c; npts[m] = points emitted; ncand[m] = candidates before
 * the cut (> max_points: the cap bit).  Entries at i >= npts[m] are not written.  nk frames <= 2^31 - 1.
 *
 * msd_cluster*: for points p[0 .. n) in float64 (x, y), n = npts[m] <= cfg->max_points <=
 * MSD_CLUSTER_MAX_POINTS, at xy[(m max_points + i) 2 + {0, 1}]:
 *   A[i][j] = (dx dx + dy dy) <= eps eps, i == j included, in float64 in that order without contraction;
 *   core[i] = popcount(A[i]) >= min_samples (sklearn's rule: the point counts itself);
 *   clusters = the connected components of the core points under A, numbered 0, 1, ... by each component's
 *   lowest-index core point; a non-core point with a core neighbour takes the lowest cluster id among its
 *   core neighbours, otherwise it is noise, -1.  These are sklearn's labels_ exactly.
 *   labels[m max_points + i] (int32), i < n; boxes (may be NULL) [(m max_points + c) 4 + {0..3}] =
 *   (x_min, y_min, x_max, y_max) over all members of cluster c, border points included; a cluster is critical
 *   when (x_max - x_min) >= critical_min_extent.  summary[m]: the counts, and status 0, or
 *   MSD_CLUSTER_STATUS_NPTS where npts[m] is outside 0 .. max_points: that image is not clustered (nothing
 *   is clamped), its counts are 0 and its labels and boxes are not written; the other images are unaffected.
 * Points must be finite.  One workgroup per image; the _dev forms enqueue only, no host loop (the label
 * propagation's rounds are bounded by n on the device).
 * eps not finite or < 0, min_samples < 1, k_lo > k_hi, k_hi >= K, a non-finite point (host form):
 * MSD_ERR_INVALID; max_points outside 1 .. MSD_CLUSTER_MAX_POINTS (host form: n above it too):
 * MSD_ERR_UNSUPPORTED.  Timing id 15 covers both kernels. */
#define MSD_CLUSTER_MAX_POINTS 512
#define MSD_CLUSTER_STATUS_NPTS 1
typedef struct {
    double eps;                 /* DBSCAN eps (detector_and_classification.py:7: 30) */
    double critical_min_extent; /* :50: 5 px */
    int32_t min_samples;        /* :7: 5 */
    int32_t max_points;         /* row stride of xy / labels / boxes; ORB's nfeatures (:12: 500) */
} msd_cluster_cfg;
typedef struct {
    int32_t n_clusters, n_critical, n_noncritical, n_noise;
    int32_t status, n_points; /* n_points: the points clustered (0 on a non-zero status) */
    int32_t reserved[2];
} msd_cluster_summary;
int msd_spec_peaks_f64_dev(msd_ctx *ctx, const double *spec, int64_t nimg, int32_t K, int64_t frames, int64_t ld,
                           int32_t k_lo, int32_t k_hi, const double *thr, double sx, double sy, int32_t max_points,
                           double *xy, int32_t *cell, int32_t *npts, int32_t *ncand);
int msd_cluster_dev(msd_ctx *ctx, const msd_cluster_cfg *cfg, const double *xy, const int32_t *npts, int64_t nimg,
                    int32_t *labels, double *boxes /* nullable */, msd_cluster_summary *summary);
/* one image, host buffers: spec dense [K][frames]; xy [max_points][2], cell [max_points] */
int msd_spec_peaks_f64(msd_ctx *ctx, const double *spec, int32_t K, int64_t frames, int32_t k_lo, int32_t k_hi,
                       double thr, double sx, double sy, int32_t max_points, double *xy, int32_t *cell,
                       int32_t *npts, int32_t *ncand);
/* one image, host buffers: xy [n][2], labels [n], boxes (may be NULL) [n][4] of which n_clusters are written */
int msd_cluster(msd_ctx *ctx, const msd_cluster_cfg *cfg, const double *xy, int32_t n, int32_t *labels,
                double *boxes /* nullable */, msd_cluster_summary *summary);

/* ------------------------------- a12: echo measurement from the device-resident spectrogram
 * One fixed-size record per detection of the batch detector, computed from the one-sided spectrogram that is
 * already in device memory (the reference stops at (start, stop, mean dB), dsp/src/main.py:30-37; these are the
 * numbers a classifier of echoes starts from).  The I/Q (two-sided) spectrogram and the live path are not
 * covered.
 *
 * Layouts: spec[f K ld + k ld + t] as msd_stft_psd_dev / msd_stft_psd_f64_dev write it; frames[f] (device
 * int64) = T of file f, <= ld; dets[f cap + i] and counts[f] as msd_detect_dev writes them; out[f cap + i] is
 * written for i < min(counts[f], cap) and left alone beyond that.
 *
 * The span, in int64.  c(s) = the lowest t >= 0 with t hop + nperseg / 2 >= s (the first frame centred at or
 * after sample s).  For detection i of file f: a0 = min(T, c(start B)), a1 = min(T, c(stop B)) (the core);
 * lo = the a1 of detection i - 1 (0 for i = 0), hi = the a0 of detection i + 1 (T for the file's last stored
 * detection); t0 = max(a0 - pre, min(lo, a0), 0), t1 = min(a1 + post, max(hi, a1), T): the padding never
 * reaches into a neighbour's core or past the file.  Columns at or past T are never read.
 *
 * Per frame t of [t0, t1), in float64, every cell converted from the stored type once, no FMA contraction:
 *   S_t = sum of rows k_lo .. k_hi in ascending k from 0.0;  N_t the same over n_lo .. n_hi;
 *   k*_t = the lowest k of [k_lo, k_hi] holding the column's maximum;
 *   with a, b, c the cells at k* - 1, k*, k* + 1 (they may lie outside the band): den = (a - 2 b) + c,
 *   delta_t = 0.5 (a - c) / den if den < 0, else 0; delta_t = 0 too when k* is row 0 or row K - 1;
 *   r_t = (k*_t - k_lo) + delta_t.
 * Per detection:
 *   p_peak = max S_t, t_peak the lowest frame attaining it; k_peak, d_peak, n_peak = k*, delta, N at t_peak;
 *   t_half_first / t_half_last = the lowest / highest frame of the span with S_t >= 0.5 p_peak;
 *   t_efold = the lowest frame after t_peak with S_t <= p_peak 0.36787944117144233 (one rounded multiply),
 *   or t1 if there is none;
 *   e_sig = sum S_t, e_noise = sum N_t, and with u = (double)(t - t0): w_r = sum S_t r_t, w_u = sum S_t u,
 *   w_uu = sum (S_t u) u, w_ur = sum (S_t u) r_t;
 *   flags: bit 0 t0 > a0 - pre, bit 1 t1 < a1 + post, bit 2 t_efold == t1, bit 3 t_peak is the first or last
 *   frame of the span.
 *   An empty span (t0 == t1): p_peak = n_peak = NaN, d_peak = 0, k_peak = -1, the sums 0, flags = bits 0-1, the
 *   four frame indices = t0.
 * The order of the six sums across frames is free (each is within (n + 3) 2^-53 sum|term| of any other order,
 * n frames); everything else is determined bit for bit.  Cells are expected finite and >= 0: NaN cells are
 * outside the contract (no fault, but the record is then unspecified).
 *
 * One wave per detection, lanes along frames; the grid is sized from nfiles and cap, never from a count read
 * back, and the _dev forms only enqueue on the context's stream.  Timing id 16.
 * MSD_ERR_INVALID: null pointers, K < 1, k_lo > k_hi or either outside [0, K), n_lo <= n_hi with either
 * outside [0, K), hop / nperseg / block_size < 1, negative padding, negative nfiles / cap, ld < frames (host
 * forms).  MSD_ERR_UNSUPPORTED: a signal or noise band of more than MSD_ECHO_MAX_BAND rows. */
#define MSD_ECHO_MAX_BAND 256
typedef struct {
    int64_t block_size;              /* B: samples per detector block (msd_det start / stop are in blocks) */
    int32_t nperseg, hop;            /* of the spectrogram: frame t covers samples [t hop, t hop + nperseg) */
    int32_t k_lo, k_hi;              /* signal band, inclusive rows of the spectrogram */
    int32_t n_lo, n_hi;              /* noise band, inclusive; n_hi < n_lo: empty (noise sums are 0) */
    int32_t pre_frames, post_frames; /* padding of the span before / after the detection, >= 0 */
} msd_echo_cfg;
typedef struct { /* 128 bytes */
    int64_t t0, t1; /* the span measured, frames [t0, t1) */
    int64_t t_peak, t_half_first, t_half_last, t_efold;
    int32_t k_peak, flags;
    double p_peak, n_peak, d_peak;
    double e_sig, e_noise, w_r, w_u, w_uu, w_ur;
} msd_echo;
int msd_echo_measure_dev(msd_ctx *ctx, const float *spec, int64_t nfiles, int32_t K, const int64_t *frames,
                         int64_t ld, const msd_det *dets, int64_t cap, const int64_t *counts,
                         const msd_echo_cfg *cfg, msd_echo *out);
/* the same over a float64 spectrogram (msd_stft_psd_f64_dev's output) */
int msd_echo_measure_f64_dev(msd_ctx *ctx, const double *spec, int64_t nfiles, int32_t K, const int64_t *frames,
                             int64_t ld, const msd_det *dets, int64_t cap, const int64_t *counts,
                             const msd_echo_cfg *cfg, msd_echo *out);
/* one file, host buffers: spec [K][ld] of which `frames` columns are valid (dense: ld = frames), the n
 * detections dets[0 .. n) and out[0 .. n) */
int msd_echo_measure(msd_ctx *ctx, const float *spec, int32_t K, int64_t frames, int64_t ld, const msd_det *dets,
                     int64_t n, const msd_echo_cfg *cfg, msd_echo *out);
int msd_echo_measure_f64(msd_ctx *ctx, const double *spec, int32_t K, int64_t frames, int64_t ld,
                         const msd_det *dets, int64_t n, const msd_echo_cfg *cfg, msd_echo *out);

/* ------------------------------------------------ a8: Welch band powers (phase 2)
 * Replaces, per processing block of dsp/src/live/backend/processor.py:177-206 and :349-369:
 *   f, psd = scipy.signal.welch(block, fs, nfft=n_fft)     (hann, nperseg 256, noverlap 128,
 *                                                           constant detrend, density, mean)
 *   P_band = np.sum(psd[(f >= lo) & (f <= hi)]);  dB = 10*log10(P_band) if P_band > 0 else -inf
 * Samples are converted to float64 and multiplied by sample_scale first (soundfile's float
 * conversion: 1/32768 for PCM16).  window: nperseg float64 (scipy get_window('hann', nperseg));
 * scale: 1/(fs*sum(win^2)) as scipy computes it.  Bands are inclusive bin ranges of
 * rfftfreq(nfft, 1/fs); hi < lo = empty band (P = 0 → -inf).  Arithmetic is float64. */
#define MSD_WELCH_MAX_BANDS 8
typedef struct {
    int32_t block_size; /* int(proc_block_sec * fs) */
    int32_t nperseg;    /* scipy default 256 (or block_size if shorter) */
    int32_t noverlap;   /* scipy default nperseg // 2 */
    int32_t nfft;       /* n_fft (>= nperseg) */
    double sample_scale;
    double scale;
    int32_t nbands;
    int32_t reserved;
    int32_t band_lo[MSD_WELCH_MAX_BANDS];
    int32_t band_hi[MSD_WELCH_MAX_BANDS];
} msd_welch_cfg;
typedef struct msd_welch_plan msd_welch_plan;
int msd_welch_plan_create(msd_ctx *ctx, const msd_welch_cfg *cfg, const double *window, msd_welch_plan **out);
void msd_welch_plan_destroy(msd_welch_plan *plan);
/* batch, device-resident (off/len device int64 arrays as for the STFT); blocks of file f:
 * (len[f] - block_size) / block_size + 1 (the reference's range(0, n - bs + 1, bs));
 * band_db[(f*nbands + j)*ld + b].  psd (may be NULL): the per-block Welch PSD of the band
 * bins, band after band, psd[(f*ld + b)*nslots + slot], nslots = sum of band widths. */
int msd_welch_bands_dev(msd_welch_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                        int64_t nfiles, int64_t max_blocks, double *band_db, int64_t ld, double *psd);
/* single signal, host buffers: band_db [nbands][nb] */
int msd_welch_bands(msd_welch_plan *plan, const void *x, int dtype, int64_t n, double *band_db, int64_t *blocks);
/* single signal, host buffers: the per-block PSD of the band bins, psd [nb][nslots] (one band
 * 0..nfft/2 and block_size = n gives scipy.signal.welch(x, fs, ...)'s whole PSD) */
int msd_welch_psd(msd_welch_plan *plan, const void *x, int dtype, int64_t n, double *psd, int64_t *blocks);
/* The whole one-sided Welch PSD of every block by a pruned float64 FFT (csrc/welch_fft.hip) instead of
 * one Goertzel recurrence per bin: scipy.signal.welch(block, fs, nperseg=, noverlap=, nfft=) for all
 * K = nfft/2 + 1 bins, and db_mean = np.mean(10*log10(row)) per block (log10(0) = -inf, as numpy's).
 * nfft a power of two in [16, 16384], any nperseg <= nfft, any noverlap < nperseg; anything else returns
 * MSD_ERR_UNSUPPORTED with nothing launched.  A block's row does not depend on the launch, the file
 * slot or the position in the batch that computed it.
 * whole one-sided Welch PSD of every block: psd[(f*ld + b)*K + k], K = nfft/2+1; db_mean[f*ld + b]
 * (may be NULL).  The plan's bands are ignored.  Entries at b >= blocks of file f are not written. */
int msd_welch_spectrum_dev(msd_welch_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                           int64_t nfiles, int64_t max_blocks, double *psd, int64_t ld, double *db_mean);
/* single signal, host buffers: psd [nb][K], db_mean (may be NULL) [nb] */
int msd_welch_spectrum(msd_welch_plan *plan, const void *x, int dtype, int64_t n, double *psd, double *db_mean,
                       int64_t *blocks);

/* The integer coefficients the exact int8-MFMA band kernels are built from (host only: no context,
 * no GPU), so that a test can restate their arithmetic in integers.  kind 0: the block plan's
 * T_n = round(w_n cos(2 pi k n / nfft) 2^54) (part 0) or round(-w_n sin(...) 2^54) (part 1);
 * kind 1: the Welch plan's T_n ~ (w_n e^{-2 pi i k n / nfft} - W_k / L) 2^53, real (part 0) or
 * imaginary part, rounded so that sum_n T_n = 0.  window: L float64 in [-1, 1]; T: L values.
 * kind 2: the refinement step's (msd_iq_delta64_dev on MSD_REFINE_INT8_MFMA) T_n = round(cos(2 pi k n /
 * nfft) 2^46) (part 0) or round(sin(...) 2^46) (part 1) for 0 <= k < nfft and n < L <= 1024; the window
 * is ignored and may be NULL.  The kernel multiplies sample n of a 256-sample sub-block by T_n (the
 * imaginary component by -T^s_n), n < 256, and combines the sub-blocks in float64. */
int msd_i8_coeffs(int kind, const double *window, int L, int nfft, int k, int part, int64_t *T);

/* --------------------------------------------- a9: live detector state machine
 * Replaces processor.py:391-507 (states aggregates.py:4-24) over per-block band dB
 * rows (signal, noise 1, noise 2):
 *   over = sig - mean(n1, n2); hist = the previous min(W, b) values of over (W = 0: all);
 *   thr = mean(hist) + k*std(hist)  (NaN on the first block), replaced by the locked
 *   threshold while Tracking, and while Detection with until > block end;
 *   Init → Detection once block_start >= init_wait; Detection → Tracking when over > thr
 *   (lock = thr + 0*std, start = block start, trigger block not in the history);
 *   Tracking appends over and ends when over < thr: emit if mean >= min_db and
 *   duration >= min_dur, then Detection(lock, until = block start + after_wait).
 * Block b starts at (b*block_size)/fs seconds.
 *
 * Every output is bit-identical to the reference's float64, signs of zero included, and every
 * comparison above is as strict as written (tests/live_cases.py):
 *   times: t0 = (b*block_size)/fs and block end t1 = ((b+1)*block_size)/fs, each one integer
 *   product divided once by fs, and until = t0 + after_wait, duration = t0 - start: separately
 *   rounded doubles, never t0 + block_size/fs and never fused.  until and a later t1 are then a
 *   rounding apart (fs 4000, block 800, wait 0.4 s: until > t1, < t1 and == t1 all occur), and a
 *   lock holds one block longer or shorter by that rounding alone; equality means "run out", as
 *   t0 == init_wait means "Init over" and duration == min_dur, mean == min_db mean "emit";
 *   over: mean(n1, n2) is (0.0 + (n1 + n2)) / 2, numpy's reduction from +0.0: n1 = n2 = -0.0
 *   gives +0.0;
 *   non-finite rows: a band dB of -inf (digital silence), +inf or NaN propagates as in IEEE
 *   arithmetic.  over = -inf or NaN never triggers and never ends Tracking by itself (NaN
 *   compares false both ways; -inf < lock ends it); while such a value lies in the window the
 *   fresh threshold is NaN and nothing triggers against it; a trigger under a lock then makes
 *   lock + 0*std = NaN and that Tracking run never ends.  db_min / db_max are Python's
 *   min / max over the history (the first element stays unless a later one compares strictly
 *   below / above: a leading NaN stays, -0.0 before +0.0 stays); a NaN mean is never emitted;
 *   buffers: thresholds / over are written at [f*ld, f*ld + nblocks[f]) only, out at
 *   [f*cap, f*cap + min(counts[f], cap)) only, whatever ld and cap; band_db is read at
 *   b < nblocks[f] only; cap = 0 and nblocks[f] = 0 are valid (count 0, status 0). */
typedef struct {
    int32_t block_size;
    int32_t avg_win_blocks; /* int(avg_win_sec / proc_block_sec), processor.py:58 */
    double fs;              /* the file's integer sample rate */
    double k_std;
    double init_wait_sec;
    double after_tracking_wait_sec;
    double min_db_mean;
    double min_dur_sec;
} msd_live_cfg;
typedef struct { /* aggregates.py:66-74 DetectedMeteor (+ the block indices) */
    int64_t start_block;
    int64_t stop_block;
    double time_start, time_stop, duration;
    double db_min, db_max, db_mean, db_std;
} msd_meteor;
/* band_db: [(f*3 + j)*ld + b] as msd_welch_bands_dev writes it (3 bands); thresholds / over
 * (may be NULL): [f*ld + b]; counts: meteors found per file (may exceed cap: only cap kept,
 * status 3). */
int msd_live_detect_dev(msd_ctx *ctx, const double *band_db, const int64_t *nblocks, int64_t nfiles, int64_t ld,
                        const msd_live_cfg *cfg, msd_meteor *out, int64_t cap, int64_t *counts, double *thresholds,
                        double *over, int32_t *status);
int msd_live_detect(msd_ctx *ctx, const double *band_db /* [3][nb] */, int64_t nb, const msd_live_cfg *cfg,
                    msd_meteor *out, int64_t cap, int64_t *count, double *thresholds, double *over);

/* ------------------------------------- a8 + a9 resumable: the live session
 * The reference station grabs 30 s of audio every 30 s around the clock
 * (meteor_detect_class/prime_detection.py:32, :148-163) and its phase-2 detector
 * (processor.py:391-507) is stateful across them.  A session holds nstreams independent
 * audio streams (receivers / frequencies of one station) and takes each stream's audio, or
 * its band-dB rows, in pushes of any length, empty ones included.  For any split of a stream
 * into pushes, the per-push outputs concatenated -- band-dB rows, over-noise values,
 * thresholds used, meteors and their order -- are bit-identical to msd_welch_bands followed
 * by msd_live_detect on the concatenated input.  Times are global: block b of a stream
 * starts at (b*block_size)/fs whichever push brought it.
 *
 * Kept on the device per stream between pushes: the detector state (msd_live_stream_state),
 * the samples that did not fill a block (< block_size), and the over-noise values a later
 * block can still read: everything from block keep = min(blocks - W, trig while Tracking) on
 * (W = avg_win_blocks; W = 0, the reference's over[-0:], keeps everything).  That tail lives
 * in hist_blocks + max_push_blocks doubles per stream.  When, after a push, more than
 * hist_blocks values would have to stay (W = 0 on a long stream; a tracking run that never
 * ends, e.g. a continuous carrier), the stream's status becomes 4 (history overflow): the
 * outputs of that push are still valid, and from then on the stream is frozen -- later pushes
 * leave its state alone, emit nothing for it (0 blocks, 0 meteors) and report 4 again --
 * until it is reset.  The other streams are unaffected.
 *
 * Per-push status[f]: 0; 3 = more meteors closed in this push than cap (only cap kept);
 * 4 = history overflow.  counts[f] = meteors closed in THIS push, at out[f*cap ..].
 *
 * The _dev pushes enqueue on the context's stream and never synchronise with the host, at
 * any push length (one wave per stream scans the push's blocks in order from the carried
 * state; there are no fixed-point rounds and no convergence flag to read).  The one exception
 * is a scratch buffer of the context growing, which can only happen on a session's first
 * pushes.  The host forms, the state getter and the history getter return after the results
 * are on the host. */
typedef struct msd_live_session msd_live_session;
typedef struct { /* one stream's carried state (aggregates.py:4-24 + the session's counters) */
    int32_t state;     /* 0 StateInitialization, 1 StateDetection, 2 StateTracking */
    int32_t status;    /* 0, or 4 = history overflow (frozen until reset) */
    int64_t blocks;    /* blocks consumed */
    int64_t trig;      /* Tracking: the global index of the block that triggered it */
    double lock;       /* locked_threshold */
    double until;      /* use_locked_threshold_until_secs */
    double t_start;    /* time_start_detection */
    int64_t meteors;   /* meteors closed since creation / reset */
    int64_t retained;  /* over-noise values kept: those of blocks [blocks - retained, blocks) */
    int64_t remainder; /* samples carried (< block_size) */
} msd_live_stream_state;
/* welch (may be NULL: the session then takes rows only) with its window as for
 * msd_welch_plan_create; it must have the three bands and cfg's block_size.  dtype: the
 * MSD_U8..MSD_F64 format of every sample push (ignored without welch).  max_push_blocks >= 1:
 * the most blocks one push may bring per stream; hist_blocks >= cfg->avg_win_blocks.
 * Device memory: 8 * (hist_blocks + 3 * max_push_blocks) bytes per stream for the detector,
 * plus (max_push_blocks + 2) blocks of samples and 24 * max_push_blocks bytes with welch. */
int msd_live_session_create(msd_ctx *ctx, const msd_live_cfg *cfg, const msd_welch_cfg *welch, const double *window,
                            int64_t nstreams, int64_t max_push_blocks, int64_t hist_blocks, int dtype,
                            msd_live_session **out);
void msd_live_session_destroy(msd_live_session *s);
/* rows: band_db[(f*3 + j)*ld + b] and device nblocks[f] as for msd_live_detect_dev; stream f
 * takes min(nblocks[f], max_blocks) rows, max_blocks <= min(ld, max_push_blocks).
 * thresholds / over (each may be NULL): the new blocks' values at [f*ld + b]; counts, status
 * (may be NULL): per stream, above.  No host synchronisation. */
int msd_live_session_push_rows_dev(msd_live_session *s, const double *band_db, const int64_t *nblocks,
                                   int64_t max_blocks, int64_t ld, msd_meteor *out, int64_t cap, int64_t *counts,
                                   double *thresholds, double *over, int32_t *status);
/* samples: stream f's new samples are x[off[f] .. off[f] + min(len[f], max_len)) (device off /
 * len as for msd_welch_bands_dev; max_len <= max_push_blocks * block_size, x may be NULL when
 * it is 0).  They follow the stream's carried remainder; the whole blocks go through the
 * Welch launch of msd_welch_bands_dev (int16: the int8 path, as there) and the detector, the
 * rest is carried.  new_blocks[f] (may be NULL): blocks completed by this push; band_db,
 * thresholds, over (each may be NULL): their rows / values, laid out as above with
 * ld >= (block_size - 1 + max_len) / block_size.  No host synchronisation. */
int msd_live_session_push_samples_dev(msd_live_session *s, const void *x, const int64_t *off, const int64_t *len,
                                      int64_t max_len, msd_meteor *out, int64_t cap, int64_t *counts,
                                      int64_t *new_blocks, double *band_db, double *thresholds, double *over,
                                      int64_t ld, int32_t *status);
/* host buffers, one stream (the others get an empty push): band_db [3][nb]; thresholds / over
 * (may be NULL) [nb]; *count may exceed cap (MSD_ERR_CAPACITY, cap meteors kept); *status (may
 * be NULL) as above.  Synchronous. */
int msd_live_session_push_rows(msd_live_session *s, int64_t stream, const double *band_db, int64_t nb,
                               msd_meteor *out, int64_t cap, int64_t *count, double *thresholds, double *over,
                               int32_t *status);
/* host buffers, one stream: n samples of the session's dtype; band_db (may be NULL) [3][ld],
 * thresholds / over (may be NULL) [ld], ld >= (block_size - 1 + n) / block_size. */
int msd_live_session_push_samples(msd_live_session *s, int64_t stream, const void *x, int64_t n, msd_meteor *out,
                                  int64_t cap, int64_t *count, int64_t *new_blocks, double *band_db,
                                  double *thresholds, double *over, int64_t ld, int32_t *status);
/* the states of streams [first, first + n) to the host.  Synchronous. */
int msd_live_session_state(msd_live_session *s, int64_t first, int64_t n, msd_live_stream_state *out);
/* one stream's retained over-noise values (those of blocks [blocks - retained, blocks), e.g.
 * StateTracking's history over[trig + 1 ..]) to the host: *n of them, at most cap copied.
 * Synchronous. */
int msd_live_session_history(msd_live_session *s, int64_t stream, double *out, int64_t cap, int64_t *n);
/* stream >= 0: that stream, -1: all, back to Init at block 0 with empty history and remainder
 * and status 0.  Enqueued on the context's stream. */
int msd_live_session_reset(msd_live_session *s, int64_t stream);

/* ------------------------------ decimating down-converter: the receiver's last stage
 * The phase-2 detector above takes 4 kHz audio in which the carrier sits at 1 kHz (the reference
 * asserts file_sample_rate == 4000 and leaves the conversion to gqrx / HDSDR).  This makes that audio
 * from what is recorded: 48 kHz audio (MSD_DDC_REAL: low-pass and decimate) or wide-band I/Q
 * (MSD_DDC_SSB: tune, low-pass, decimate and take the single-sideband audio, a Weaver demodulator).
 *
 * Contract.  x[n]: one stream's samples, n the global sample index (int64, from 0); h[0 .. ntaps-1]: real
 * float64 taps, ntaps odd, c = (ntaps-1)/2; D = decim.  Samples outside what a call or a stream has seen
 * count as zero.
 *   REAL (MSD_I16 or MSD_F32):  v[m] = sum_{k=0}^{ntaps-1} h[k] x[m D + c - k],  y[m] = gain v[m].
 *   SSB (MSD_CI16 or MSD_CF32, interleaved I, Q):  z[n] = x[n] e^{-2 pi i r(n)/q},  r(n) = (n p) mod q exactly
 *   in integers,  p/q = shift_num/shift_den in lowest terms (cycles per input sample);  v[m] as above over z;
 *   y[m] = gain Re(i^m v[m]).  With shift = (f_signal - f_tone + fs_out/4)/fs_in and a low-pass below
 *   fs_out/4 a carrier at f_signal comes out as a real tone at f_tone and the other sideband is rejected.
 * Outputs.  A batch row holding samples [pos0, pos0+N) emits every m with pos0 <= m D < pos0+N:
 * ceil((pos0+N)/D) - ceil(pos0/D) of them.  A stream that has received N_tot samples has emitted every m
 * with m D + c < N_tot; msd_ddc_flush emits the rest, m D < N_tot, with zeros for the samples to come; a
 * flushed stream must be reset before it is pushed again.  msd_ddc_reset(plan, stream, pos0) clears the
 * history and sets the stream's position (stream -1: all), so a stream may start anywhere.
 * Output dtype: MSD_F64, or MSD_I16 = rint(y) (ties to even) saturated to [-32768, 32767].
 * Arithmetic: float64, no contraction but the kernel's explicit FMAs.  The summation order of an output
 * is a function of (ntaps, D) alone (csrc/ddc_plan.h), never of tile, grid, chunking or entry point:
 * pushes of any lengths followed by flush equal one msd_ddc_run over the concatenation bit for bit, and a
 * row with c samples of halo on each side equals the whole stream on its interior outputs bit for bit.
 * Error: |y - y_exact| <= chain u gain S_m, u = 2^-53, S_m = sum_k |h_k| |x_{m D + c - k}|, chain =
 * msd_ddc_chain (counted from the kernel's code, csrc/ddc_plan.h).
 * Limits: 1 <= decim <= 1024; ntaps odd in 1 .. 4095; reduced 1 <= q <= 2^24, 0 <= p < q; positions up to
 * 2^62.  REAL with p != 0 and sizes outside the limits: MSD_ERR_UNSUPPORTED; an even ntaps, a dtype that
 * does not fit the mode, a bad out_dtype: MSD_ERR_INVALID.
 * Streams: nstreams >= 0 independent streams whose state lives in the plan on the device: the position
 * and the last ntaps-1 raw samples (raw, not mixed: the phase comes from the global index).  A stream
 * keeps the dtype of its first push until it is reset.  max_push: the most samples one push brings per
 * stream (longer device pushes are cut to it).
 * _dev calls only enqueue on the context's stream.  off / len / pos0: device int64 arrays (samples of
 * dtype; a complex sample is one sample).  y: rows of ld_out outputs of the plan's out_dtype; out_len:
 * device int64, the row's full count.  Only the first ld_out outputs of a row are written and nothing
 * past a row's count is touched; msd_ddc_push_dev needs ld_out >= ceil(max_push / D).
 * The host forms return MSD_ERR_CAPACITY (with *out_len set, nothing copied) when cap is too small. */
#define MSD_DDC_REAL 0
#define MSD_DDC_SSB 1
typedef struct {
    int32_t mode, decim, ntaps, out_dtype;
    int64_t shift_num, shift_den;
    double gain;
} msd_ddc_cfg;
typedef struct msd_ddc_plan msd_ddc_plan;
int msd_ddc_plan_create(msd_ctx *ctx, const msd_ddc_cfg *cfg, const double *taps, int64_t nstreams, int64_t max_push,
                        msd_ddc_plan **out);
void msd_ddc_plan_destroy(msd_ddc_plan *plan);
/* host only, no context: the first output index and the output count of a row [pos0, pos0 + n) */
int msd_ddc_out_len(const msd_ddc_cfg *cfg, int64_t pos0, int64_t n, int64_t *m0, int64_t *count);
/* host only, no context: the rounding chain of the bound above */
int msd_ddc_chain(const msd_ddc_cfg *cfg, double *chain);
/* independent rows: row r holds samples [pos0[r], pos0[r] + len[r]) at x[off[r] ..] */
int msd_ddc_run_dev(msd_ddc_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                    const int64_t *pos0, int64_t nrows, void *y, int64_t ld_out, int64_t *out_len);
/* one row, host buffers */
int msd_ddc_run(msd_ddc_plan *plan, const void *x, int dtype, int64_t n, int64_t pos0, void *y, int64_t cap,
                int64_t *out_len);
/* all nstreams: stream f's new samples are x[off[f] .. off[f] + min(len[f], max_push)) */
int msd_ddc_push_dev(msd_ddc_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len, void *y,
                     int64_t ld_out, int64_t *out_len);
/* one stream, host buffers, n <= max_push */
int msd_ddc_push(msd_ddc_plan *plan, int64_t stream, const void *x, int dtype, int64_t n, void *y, int64_t cap,
                 int64_t *out_len);
/* one stream, host buffers: at most ceil(c / D) + 1 outputs */
int msd_ddc_flush(msd_ddc_plan *plan, int64_t stream, void *y, int64_t cap, int64_t *out_len);
int msd_ddc_reset(msd_ddc_plan *plan, int64_t stream, int64_t pos0);

/* ------------------------------ rational-ratio resampler: the down-converter at any ratio up / down
 * The down-converter above decimates by an integer.  This one resamples by L / M = up / down (a polyphase
 * filter), so that the detector's 4 kHz audio also comes from 6 kHz archive files (2/3), 44.1 kHz sound
 * cards (40/441) and 250 kHz I/Q (2/125), with the same modes, dtypes, streams and guarantees.
 *
 * Contract.  L = up, M = down, gcd(L, M) = 1; h[0 .. ntaps-1]: real float64 taps, ntaps odd, c = (ntaps-1)/2.
 * Samples outside what a call or a stream has seen count as zero.  Output m:
 *   t = m M + c,  phi = t mod L,  n0 = t div L,
 *   v[m] = sum_{i=0}^{I_phi - 1} h[phi + i L] z[n0 - i],  I_phi = ceil((ntaps - phi) / L); a branch with no tap
 *   (phi >= ntaps) gives exactly 0;
 *   z = x (mode MSD_DDC_REAL) or x[n] e^{-2 pi i r(n)/q}, r(n) = (n p) mod q exactly in integers (MSD_DDC_SSB),
 *   p/q = shift_num/shift_den in lowest terms, cycles per input sample;
 *   y[m] = gain v[m] (REAL) or gain Re(i^m v[m]) (SSB).
 * In float64 this is scipy.signal.upfirdn(h, x, L, M) read at lag c; REAL at pos0 = 0 is
 * scipy.signal.resample_poly(x, L, M, window=h/L).  With up = 1 the definition is msd_ddc's (the bits need
 * not be).
 * Outputs.  A batch row holding samples [pos0, pos0+N) emits every m with pos0 L <= m M < (pos0+N) L:
 * ceil((pos0+N) L / M) - ceil(pos0 L / M) of them.  A stream that has received N_tot samples has emitted every
 * m with m M + c < N_tot L; msd_resamp_flush emits the rest, m M < N_tot L, with zeros for the samples to come
 * (at most ceil(c / M) + 1 outputs); a flushed stream refuses pushes until it is reset.
 * msd_resamp_reset(plan, stream, pos0) clears the history and sets the position (stream -1: all).
 * Per-stream state on the device: the position and the last ceil(ntaps / L) - 1 raw (unmixed) samples, which
 * suffice because the oldest input of an output not yet emitted is >= N_tot - ceil(ntaps / L) + 1.
 * Output dtype: MSD_F64, or MSD_I16 = rint(y) (ties to even) saturated to [-32768, 32767].
 * Arithmetic: float64, no contraction but the kernel's explicit FMAs.  The summation order of an output is a
 * function of (ntaps, L, M) and the output's branch phi alone (csrc/resamp_plan.h), never of tile, grid,
 * chunking or entry point: pushes of any lengths followed by flush equal one msd_resamp_run over the
 * concatenation bit for bit, a row with enough halo (ceil(ntaps / L) samples on each side) equals the whole
 * stream on its interior outputs bit for bit, and streams pushed together equal each alone.
 * Non-finite MSD_F32 / MSD_CF32 samples: an output is the IEEE-754 value of its own sum and of nothing else
 * (no padded tap or sample of another output's window takes part): an output whose window
 * n0 - I_phi + 1 .. n0 holds no such sample is what it is with that sample replaced by 0, one whose window
 * holds one is not finite (REAL: +-inf where every infinite product has one sign, NaN otherwise, e.g. where
 * the tap that meets it is 0), and a branch with no tap still gives 0.  As int16, NaN becomes 0.
 * Error: |y - y_exact| <= chain u |gain| S_m, u = 2^-53, S_m = sum_i |h[phi + i L]| |x[n0 - i]|, chain =
 * msd_resamp_chain (counted from the kernel's code, csrc/resamp_plan.h); chain <= 10 + ceil(ntaps / L) + G - 1
 * with G the plan's partial sums per output.
 * Limits: 1 <= up <= 256; 1 <= down <= 1024; ntaps odd in 1 .. 4095; q, p and the dtypes as for msd_ddc;
 * (pos0 + n) up <= 2^62.  gcd(up, down) != 1, an even ntaps, a dtype that does not fit the mode, a bad
 * out_dtype: MSD_ERR_INVALID; sizes outside the limits or REAL with a shift: MSD_ERR_UNSUPPORTED.
 * Streams, max_push, the _dev calls' arguments and the host forms' MSD_ERR_CAPACITY are msd_ddc's;
 * msd_resamp_push_dev needs ld_out >= ceil(max_push L / M) + 1.  Timing id 14. */
typedef struct {
    int32_t mode, up, down, ntaps, out_dtype, reserved;
    int64_t shift_num, shift_den;
    double gain;
} msd_resamp_cfg;
typedef struct msd_resamp_plan msd_resamp_plan;
int msd_resamp_plan_create(msd_ctx *ctx, const msd_resamp_cfg *cfg, const double *taps, int64_t nstreams,
                           int64_t max_push, msd_resamp_plan **out);
void msd_resamp_plan_destroy(msd_resamp_plan *plan);
/* host only, no context: the first output index and the output count of a row [pos0, pos0 + n) */
int msd_resamp_out_len(const msd_resamp_cfg *cfg, int64_t pos0, int64_t n, int64_t *m0, int64_t *count);
/* host only, no context: the rounding chain of the bound above */
int msd_resamp_chain(const msd_resamp_cfg *cfg, double *chain);
/* independent rows: row r holds samples [pos0[r], pos0[r] + len[r]) at x[off[r] ..] */
int msd_resamp_run_dev(msd_resamp_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                       const int64_t *pos0, int64_t nrows, void *y, int64_t ld_out, int64_t *out_len);
/* one row, host buffers */
int msd_resamp_run(msd_resamp_plan *plan, const void *x, int dtype, int64_t n, int64_t pos0, void *y, int64_t cap,
                   int64_t *out_len);
/* all nstreams: stream f's new samples are x[off[f] .. off[f] + min(len[f], max_push)) */
int msd_resamp_push_dev(msd_resamp_plan *plan, const void *x, int dtype, const int64_t *off, const int64_t *len,
                        void *y, int64_t ld_out, int64_t *out_len);
/* one stream, host buffers, n <= max_push */
int msd_resamp_push(msd_resamp_plan *plan, int64_t stream, const void *x, int dtype, int64_t n, void *y, int64_t cap,
                    int64_t *out_len);
/* one stream, host buffers: at most ceil(c / M) + 1 outputs */
int msd_resamp_flush(msd_resamp_plan *plan, int64_t stream, void *y, int64_t cap, int64_t *out_len);
int msd_resamp_reset(msd_resamp_plan *plan, int64_t stream, int64_t pos0);

/* ------------------------------------------- a1 / §8(f)1: WAV ingest and uploads
 * scipy.io.wavfile.read semantics for the reference's files (dsp/src/main.py:249; the rules in
 * csrc/wav_parse.h): RIFF little-endian; the sample container is nBlockAlign / nChannels; PCM
 * 1..8 bits → u8, 2-byte → i16, 3-byte → i32 (sample in the top 3 bytes), 4-byte → i32;
 * IEEE float 32 / 64; WAVE_FORMAT_EXTENSIBLE.  msd_wav_read decodes frames
 * [frame0, frame0+nframes) of one channel (channel >= 0) or all (channel = -1, interleaved)
 * with pread straight into dst (host memory; pinned memory from msd_host_alloc lets the
 * upload run asynchronously).  Thread-safe (no shared state). */
typedef struct {
    int32_t rate, channels, bits, format; /* format: 1 PCM, 3 IEEE float */
    int32_t dtype;                        /* MSD_* of the decoded samples */
    int32_t reserved;                     /* the file's bytes per sample (container) */
    int64_t frames;                       /* frames (samples per channel) */
    int64_t data_offset, data_bytes;
} msd_wav_info;
int msd_wav_probe(const char *path, msd_wav_info *info);
int msd_wav_read(const char *path, int32_t channel, int64_t frame0, int64_t nframes, void *dst, int64_t dst_bytes,
                 msd_wav_info *info);
int msd_host_alloc(msd_ctx *ctx, size_t bytes, void **ptr); /* pinned (page-locked) */
int msd_host_free(msd_ctx *ctx, void *ptr);
/* upload on the context's copy stream (overlaps the compute stream) */
int msd_memcpy_h2d_async(msd_ctx *ctx, void *dst, const void *src, size_t bytes);
/* direction 0: work enqueued on the compute stream from now on waits for the uploads enqueued
 * so far; 1: uploads enqueued from now on wait for the compute enqueued so far */
int msd_fence(msd_ctx *ctx, int direction);
int msd_copy_synchronize(msd_ctx *ctx);
/* work enqueued on waiter's stream from now on waits for the work enqueued on signaler's
 * stream so far (two contexts of one device: independent stages of a step run concurrently,
 * e.g. the STFT beside block_delta -> detect in BatchPipeline; no reference counterpart) */
int msd_stream_wait(msd_ctx *waiter, msd_ctx *signaler);

/* ------------------------------------------ multi-GPU: per-hour count reduction
 * RCCL (loaded at run time from librccl.so.1), one communicator per (process, GPU). */
#define MSD_COMM_ID_BYTES 128
int msd_comm_get_unique_id(char *id /* MSD_COMM_ID_BYTES */);
int msd_comm_init(msd_ctx *ctx, int nranks, const char *id, int rank, msd_comm **out);
void msd_comm_destroy(msd_comm *comm);
/* in-place sum of n int64 on the device, on the context stream */
int msd_comm_allreduce_i64(msd_comm *comm, int64_t *dbuf, int64_t n);
/* recv[r*bytes .. (r+1)*bytes) = rank r's send (device buffers, context stream) — the C5
 * stream detector's halo / chunk-sum / shard-state exchange */
int msd_comm_allgather(msd_comm *comm, const void *dsend, void *drecv, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* MSDSP_H */
