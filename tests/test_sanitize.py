"""CPU sanitizer target: the host C++ that parses untrusted WAV
files or plans device work, built with g++ -fsanitize=address,undefined
(`make -C meteor-scatter_amd/csrc sanitize` -> build/host_check_san, csrc/host_check.cpp) and run on

* malformed WAV files next to scipy.io.wavfile.read (scipy/io/wavfile.py:568-733), the reader
  the reference uses (dsp/src/main.py:249): the two either both refuse a file or both return the
  same samples; libmsdsp's own reader (msd_wav_probe / msd_wav_read, the same wav_parse.h) agrees;
* a seeded fuzz of mutated / truncated WAV images decoded in memory (exact-size buffers: any read
  past the image is an AddressSanitizer report), numpy's np.sum leaf programs and the float64
  refinement planner;
* the int8-MFMA kernels' coefficient digits and fragment order (i8_digits.h).

A sanitizer report aborts the harness (-fno-sanitize-recover=all), which fails the test."""
import os
import shutil
import struct
import subprocess
import warnings

import numpy as np
import pytest
import scipy.io.wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meteor-scatter_amd", "csrc")
EXE = os.path.join(CSRC, "build", "host_check_san")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed for the sanitizer build")


@pytest.fixture(scope="module")
def harness():
    # one build at a time: pytest-xdist workers would otherwise exec a half-linked binary
    import fcntl
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    with open(os.path.join(CSRC, "build", ".sanitize.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", CSRC, "sanitize"], check=True, capture_output=True)
    return EXE


def run(harness, *args):
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, *map(str, args)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, f"sanitizer / check failure:\n{r.stdout}\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.strip()


def fnv1a(b: bytes) -> int:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def riff(chunks, riff_size=None):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body) if riff_size is None else riff_size) + body


def chunk(cid, payload, size=None):
    pad = b"\x00" if len(payload) % 2 else b""
    return cid + struct.pack("<I", len(payload) if size is None else size) + payload + pad


def fmt(tag=1, ch=1, rate=48000, cont=2, bits=16, byte_rate=None, extra=b""):
    br = rate * cont * ch if byte_rate is None else byte_rate
    return chunk(b"fmt ", struct.pack("<HHIIHH", tag, ch, rate, br, cont * ch, bits) + extra)


EXT_TAIL = b"\x00\x00\x10\x00\x80\x00\x00\xAA\x00\x38\x9B\x71"
rng = np.random.default_rng(7)
S16 = rng.integers(-32768, 32767, 600).astype("<i2").tobytes()  # 300 stereo / 600 mono samples
S24 = rng.integers(0, 256, 3 * 301, dtype=np.uint8).tobytes()   # 301 mono 24-bit samples (odd size)

CASES = {
    "mono16": riff([fmt(), chunk(b"data", S16)]),
    "stereo16": riff([fmt(ch=2), chunk(b"data", S16)]),
    "u8": riff([fmt(cont=1, bits=8), chunk(b"data", S16[:301])]),
    "f32": riff([fmt(tag=3, cont=4, bits=32), chunk(b"data", np.linspace(-1, 1, 77, dtype="<f4").tobytes())]),
    "f64": riff([fmt(tag=3, cont=8, bits=64, ch=2), chunk(b"data", np.linspace(-1, 1, 64, dtype="<f8").tobytes())]),
    "pcm24_odd_frames": riff([fmt(cont=3, bits=24), chunk(b"data", S24)]),
    "extensible16": riff([fmt(tag=0xFFFE, extra=struct.pack("<HHI", 22, 16, 0) + struct.pack("<I", 1) + EXT_TAIL),
                          chunk(b"data", S16)]),
    "extensible_bad_guid": riff([fmt(tag=0xFFFE, extra=struct.pack("<HHI", 22, 16, 0) + struct.pack("<I", 1) +
                                     b"\x11" * 12), chunk(b"data", S16)]),
    "extensible_short_cb": riff([fmt(tag=0xFFFE, extra=struct.pack("<HHI", 20, 16, 0) + b"\x00" * 16),
                                 chunk(b"data", S16)]),
    "odd_list_padding": riff([fmt(), chunk(b"LIST", b"abcde"), chunk(b"data", S16)]),
    "odd_unknown_chunk": riff([chunk(b"junk", b"xyz"), fmt(ch=2), chunk(b"data", S16)]),
    "fmt_size_lt_16": riff([chunk(b"fmt ", struct.pack("<HHIIH", 1, 1, 48000, 96000, 2)), chunk(b"data", S16)]),
    "zero_channels": riff([fmt(ch=0, byte_rate=0), chunk(b"data", S16)]),
    "bad_byte_rate": riff([fmt(byte_rate=12345), chunk(b"data", S16)]),
    "no_fmt_before_data": riff([chunk(b"data", S16), fmt()]),
    "data_past_eof_mono": riff([fmt(), chunk(b"data", S16)[:-100]]),
    "data_past_eof_stereo_partial_frame": riff([fmt(ch=2), chunk(b"data", S16)[:-2]]),
    "data_size_ffffffff": riff([fmt(), b"data" + struct.pack("<I", 0xFFFFFFFF) + S16]),
    "data_size_ffffffff_stereo": riff([fmt(ch=2), b"data" + struct.pack("<I", 0xFFFFFFFF) + S16]),
    "chunk_size_ffffffff_before_data": riff([fmt(), chunk(b"LIST", b"ab", size=0xFFFFFFFF), chunk(b"data", S16)]),
    "truncated_chunk_header": riff([fmt(), b"LIS"]),
    "truncated_chunk_size": riff([fmt(), b"LIST\x05\x00"]),
    "truncated_fmt_body": riff([fmt()[:20]]),
    "riff_size_excludes_data": riff([fmt(), chunk(b"data", S16)], riff_size=4 + 24),
    "riff_size_small_but_covers_data": riff([fmt(), chunk(b"data", S16)], riff_size=4 + 24 + 8),
    "riff_size_ffffffff": riff([fmt(), chunk(b"data", S16)], riff_size=0xFFFFFFFF),
    "empty_data": riff([fmt(), chunk(b"data", b"")]),
    "not_riff": b"JUNK" + b"\x00" * 40,
    "short_file": b"RIFF\x00",
    "int64_pcm": riff([fmt(cont=8, bits=64), chunk(b"data", S16[:64])]),
}
# scipy reads these; libmsdsp refuses them (wav_parse.h "Differences"), so they are excluded from
# the both-agree check and asserted as refusals instead
OURS_REFUSE = {"int64_pcm"}


def scipy_read(path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            fs, data = scipy.io.wavfile.read(path)
        except Exception as e:  # noqa: BLE001 -- any refusal (ValueError, struct.error, ZeroDivisionError, ...)
            return None, repr(e)
    return fs, np.ascontiguousarray(data)


@pytest.mark.parametrize("name", sorted(CASES))
def test_malformed_wav_matches_scipy(harness, tmp_path, name):
    p = tmp_path / f"{name}.wav"
    p.write_bytes(CASES[name])
    out = run(harness, "wav", p)
    fs, data = scipy_read(p)
    if name in OURS_REFUSE:
        assert out.startswith("err"), out
        return
    if fs is None:
        assert out.startswith("err"), f"scipy refuses ({data}) but the parser reads: {out}"
        return
    assert out.startswith("ok"), f"scipy reads {data.shape} {data.dtype} but the parser refuses: {out}"
    f = out.split()
    rate, channels, frames, digest = int(f[1]), int(f[2]), int(f[7]), int(f[10], 16)
    assert rate == fs and frames == data.shape[0] and channels == (1 if data.ndim == 1 else data.shape[1])
    assert digest == fnv1a(data.tobytes()), "decoded samples differ from scipy's"
    # libmsdsp's reader (the product path, same header) returns scipy's array
    from meteorgpu import ingest
    fs2, y = ingest.read(p)
    assert fs2 == fs and y.dtype == data.dtype and y.shape == data.shape
    np.testing.assert_array_equal(y, data)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_under_sanitizers(harness, seed):
    out = run(harness, "fuzz", seed, 4000)
    assert out.startswith("ok"), out
    parsed = int(out.split()[1])
    assert parsed > 1000  # most mutations still parse: the decode path is exercised


@pytest.mark.parametrize("n", [0, 1, 127, 128, 129, 8191, 8192, 8193, 22500, 3 * 8192 + 17])
def test_np_program_under_sanitizers(harness, n):
    assert run(harness, "program", n).startswith("ok")


def test_refine_plan_under_sanitizers(harness):
    # C5 (bins 21..22 and -65..-63: 9 needed bins, blocks of 1024, 4 per frame)
    assert run(harness, "refine", 4096, 1024, 21, 22, -65, -63, 10 ** 6, 0, 10, 40, 90).split()[1:4] == ["9", "1024", "4"]
    # a hop that is not a power of two (blocks of gcd(4096, 1000) = 8 samples)
    assert run(harness, "refine", 4096, 1000, 21, 22, -65, -63, 10 ** 6, 3, 9).split()[2:4] == ["8", "512"]
    # the 16-lane Goertzel rows only for D % 64 == 0: D = 1024 rows, D = 500 (N 1000,
    # hop 500) and D = 96 (N 192, hop 96) the one-lane direct path
    assert run(harness, "refine", 4096, 1024, 21, 22, -65, -63, 10 ** 6, 0, 10).split()[6] == "1"
    for n, hop, d in ((1000, 500, "500"), (192, 96, "96"), (4096, 2560, "512")):
        out = run(harness, "refine", n, hop, 3, 4, -9, -7, 10 ** 5, 0, 10).split()
        assert out[0] == "ok" and out[2] == d and out[6] == ("1" if int(d) % 64 == 0 else "0"), out
    # refused, not crashed: overlapping ranges, a band outside the spectrum, frames past the samples
    assert run(harness, "refine", 4096, 1024, 21, 22, -65, -63, 10 ** 6, 0, 10, 5, 20).startswith("err")
    assert run(harness, "refine", 4096, 1024, 21, 5000, -65, -63, 10 ** 6, 0, 10).startswith("err")
    assert run(harness, "refine", 4096, 1024, 21, 22, -65, -63, 8192, 0, 10).startswith("err")
    assert run(harness, "refine", 131072, 1024, 21, 22, -65, -63, 10 ** 7, 0, 10).startswith("err")  # > 65536


# guided_chunks' constants at its two call sites: (div, cmin, multiple, merge_short_tail)
SCHED_STFT1024 = (2, 2, 1, 1)
SCHED_CSTFT = (4, 16, 4, 0)
# Chunk bounds recorded from the two loops guided_chunks replaced (stft1024.hip's launch_fast_t over
# tiles, cstft.hip's msd_cstft_psd_fsums_dev over frames), per (constants, total, wgs).  The long
# ones are kept as runs of equal chunk sizes, "SIZExCOUNT ...".
SCHED_BOUNDS = {
    (SCHED_STFT1024, 1, 1): [0, 1],
    (SCHED_STFT1024, 5, 1): [0, 2, 5],
    (SCHED_STFT1024, 7, 1): [0, 3, 5, 7],
    (SCHED_STFT1024, 10, 2): [0, 2, 4, 6, 8, 10],
    (SCHED_CSTFT, 1, 1): [0, 1],
    (SCHED_CSTFT, 100, 1): [0, 28, 48, 64, 80, 96, 100],
}
SCHED_RUNS = {
    (SCHED_STFT1024, 11 * 1440, 256): (
        "30x17 29x17 28x18 27x19 26x20 25x21 24x21 23x22 22x23 21x25 20x25 19x27 18x29 17x30 16x32 15x34 "
        "14x36 13x40 12x42 11x47 10x51 9x57 8x63 7x74 6x85 5x102 4x128 3x170 2x766 3x1 "),
    (SCHED_CSTFT, 4 * 1021 + 3, 768): "16x255 7x1",
    (SCHED_CSTFT, 16200000, 1024): (
        "3956x3 3952x4 3948x4 3944x4 3940x4 3936x4 3932x5 3928x4 3924x4 3920x4 3916x4 3912x4 3908x5 3904x4 "
        "3900x4 3896x4 3892x4 3888x5 3884x4 3880x4 3876x4 3872x5 3868x4 3864x4 3860x4 3856x5 3852x4 3848x4 "
        "3844x4 3840x5 3836x4 3832x4 3828x4 3824x5 3820x4 3816x4 3812x5 3808x4 3804x4 3800x5 3796x4 3792x4 "
        "3788x4 3784x5 3780x4 3776x4 3772x5 3768x4 3764x5 3760x4 3756x4 3752x5 3748x4 3744x4 3740x5 3736x4 "
        "3732x4 3728x5 3724x4 3720x5 3716x4 3712x5 3708x4 3704x4 3700x5 3696x4 3692x5 3688x4 3684x5 3680x4 "
        "3676x4 3672x5 3668x4 3664x5 3660x4 3656x5 3652x4 3648x5 3644x4 3640x5 3636x4 3632x5 3628x4 3624x5 "
        "3620x4 3616x5 3612x4 3608x5 3604x5 3600x4 3596x5 3592x4 3588x5 3584x4 3580x5 3576x4 3572x5 3568x5 "
        "3564x4 3560x5 3556x4 3552x5 3548x5 3544x4 3540x5 3536x5 3532x4 3528x5 3524x4 3520x5 3516x5 3512x4 "
        "3508x5 3504x5 3500x5 3496x4 3492x5 3488x5 3484x4 3480x5 3476x5 3472x4 3468x5 3464x5 3460x5 3456x4 "
        "3452x5 3448x5 3444x5 3440x4 3436x5 3432x5 3428x5 3424x4 3420x5 3416x5 3412x5 3408x5 3404x4 3400x5 "
        "3396x5 3392x5 3388x5 3384x5 3380x4 3376x5 3372x5 3368x5 3364x5 3360x5 3356x5 3352x5 3348x4 3344x5 "
        "3340x5 3336x5 3332x5 3328x5 3324x5 3320x5 3316x5 3312x5 3308x5 3304x5 3300x5 3296x5 3292x5 3288x5 "
        "3284x5 3280x5 3276x5 3272x5 3268x5 3264x5 3260x5 3256x5 3252x5 3248x5 3244x5 3240x5 3236x5 3232x5 "
        "3228x5 3224x5 3220x5 3216x5 3212x5 3208x5 3204x6 3200x5 3196x5 3192x5 3188x5 3184x5 3180x5 3176x6 "
        "3172x5 3168x5 3164x5 3160x5 3156x5 3152x6 3148x5 3144x5 3140x5 3136x6 3132x5 3128x5 3124x5 3120x5 "
        "3116x6 3112x5 3108x5 3104x6 3100x5 3096x5 3092x5 3088x6 3084x5 3080x5 3076x6 3072x5 3068x5 3064x6 "
        "3060x5 3056x5 3052x6 3048x5 3044x6 3040x5 3036x5 3032x6 3028x5 3024x6 3020x5 3016x5 3012x6 3008x5 "
        "3004x6 3000x5 2996x6 2992x5 2988x6 2984x5 2980x6 2976x5 2972x6 2968x5 2964x6 2960x5 2956x6 2952x5 "
        "2948x6 2944x5 2940x6 2936x6 2932x5 2928x6 2924x5 2920x6 2916x6 2912x5 2908x6 2904x5 2900x6 2896x6 "
        "2892x5 2888x6 2884x6 2880x6 2876x5 2872x6 2868x6 2864x5 2860x6 2856x6 2852x6 2848x5 2844x6 2840x6 "
        "2836x6 2832x5 2828x6 2824x6 2820x6 2816x6 2812x5 2808x6 2804x6 2800x6 2796x6 2792x6 2788x6 2784x5 "
        "2780x6 2776x6 2772x6 2768x6 2764x6 2760x6 2756x6 2752x6 2748x6 2744x6 2740x6 2736x6 2732x6 2728x6 "
        "2724x6 2720x6 2716x6 2712x6 2708x6 2704x6 2700x6 2696x6 2692x6 2688x6 2684x6 2680x6 2676x7 2672x6 "
        "2668x6 2664x6 2660x6 2656x6 2652x7 2648x6 2644x6 2640x6 2636x6 2632x7 2628x6 2624x6 2620x6 2616x7 "
        "2612x6 2608x6 2604x6 2600x7 2596x6 2592x6 2588x7 2584x6 2580x6 2576x7 2572x6 2568x6 2564x7 2560x6 "
        "2556x7 2552x6 2548x6 2544x7 2540x6 2536x7 2532x6 2528x7 2524x6 2520x7 2516x6 2512x7 2508x6 2504x7 "
        "2500x6 2496x7 2492x7 2488x6 2484x7 2480x6 2476x7 2472x7 2468x6 2464x7 2460x7 2456x6 2452x7 2448x7 "
        "2444x6 2440x7 2436x7 2432x6 2428x7 2424x7 2420x7 2416x7 2412x6 2408x7 2404x7 2400x7 2396x7 2392x6 "
        "2388x7 2384x7 2380x7 2376x7 2372x7 2368x7 2364x7 2360x7 2356x7 2352x7 2348x7 2344x7 2340x7 2336x7 "
        "2332x7 2328x7 2324x7 2320x7 2316x7 2312x7 2308x7 2304x7 2300x7 2296x7 2292x8 2288x7 2284x7 2280x7 "
        "2276x7 2272x7 2268x8 2264x7 2260x7 2256x7 2252x8 2248x7 2244x7 2240x8 2236x7 2232x7 2228x8 2224x7 "
        "2220x7 2216x8 2212x7 2208x8 2204x7 2200x7 2196x8 2192x7 2188x8 2184x7 2180x8 2176x7 2172x8 2168x7 "
        "2164x8 2160x8 2156x7 2152x8 2148x7 2144x8 2140x8 2136x7 2132x8 2128x8 2124x8 2120x7 2116x8 2112x8 "
        "2108x8 2104x7 2100x8 2096x8 2092x8 2088x8 2084x7 2080x8 2076x8 2072x8 2068x8 2064x8 2060x8 2056x8 "
        "2052x8 2048x8 2044x8 2040x8 2036x8 2032x8 2028x8 2024x8 2020x8 2016x8 2012x9 2008x8 2004x8 2000x8 "
        "1996x8 1992x9 1988x8 1984x8 1980x8 1976x9 1972x8 1968x8 1964x9 1960x8 1956x8 1952x9 1948x8 1944x9 "
        "1940x8 1936x8 1932x9 1928x8 1924x9 1920x9 1916x8 1912x9 1908x8 1904x9 1900x8 1896x9 1892x9 1888x8 "
        "1884x9 1880x9 1876x9 1872x8 1868x9 1864x9 1860x9 1856x8 1852x9 1848x9 1844x9 1840x9 1836x9 1832x9 "
        "1828x9 1824x9 1820x9 1816x9 1812x9 1808x9 1804x9 1800x9 1796x9 1792x9 1788x10 1784x9 1780x9 1776x9 "
        "1772x9 1768x10 1764x9 1760x9 1756x10 1752x9 1748x9 1744x10 1740x9 1736x10 1732x9 1728x9 1724x10 "
        "1720x10 1716x9 1712x10 1708x9 1704x10 1700x9 1696x10 1692x10 1688x10 1684x9 1680x10 1676x10 1672x10 "
        "1668x9 1664x10 1660x10 1656x10 1652x10 1648x10 1644x10 1640x10 1636x10 1632x10 1628x10 1624x10 "
        "1620x10 1616x10 1612x10 1608x11 1604x10 1600x10 1596x10 1592x11 1588x10 1584x10 1580x11 1576x10 "
        "1572x10 1568x11 1564x10 1560x11 1556x10 1552x11 1548x11 1544x10 1540x11 1536x10 1532x11 1528x11 "
        "1524x11 1520x10 1516x11 1512x11 1508x11 1504x11 1500x11 1496x11 1492x11 1488x11 1484x11 1480x11 "
        "1476x11 1472x11 1468x11 1464x11 1460x12 1456x11 1452x11 1448x11 1444x12 1440x11 1436x12 1432x11 "
        "1428x11 1424x12 1420x11 1416x12 1412x12 1408x11 1404x12 1400x12 1396x11 1392x12 1388x12 1384x12 "
        "1380x12 1376x12 1372x12 1368x11 1364x13 1360x12 1356x12 1352x12 1348x12 1344x12 1340x12 1336x13 "
        "1332x12 1328x12 1324x13 1320x12 1316x12 1312x13 1308x12 1304x13 1300x13 1296x12 1292x13 1288x13 "
        "1284x12 1280x13 1276x13 1272x13 1268x13 1264x13 1260x13 1256x13 1252x13 1248x13 1244x13 1240x13 "
        "1236x14 1232x13 1228x13 1224x14 1220x13 1216x14 1212x13 1208x14 1204x13 1200x14 1196x14 1192x13 "
        "1188x14 1184x14 1180x14 1176x14 1172x14 1168x14 1164x14 1160x14 1156x14 1152x14 1148x15 1144x14 "
        "1140x14 1136x15 1132x14 1128x15 1124x14 1120x15 1116x15 1112x14 1108x15 1104x15 1100x15 1096x15 "
        "1092x15 1088x15 1084x15 1080x15 1076x15 1072x16 1068x15 1064x15 1060x16 1056x15 1052x16 1048x16 "
        "1044x15 1040x16 1036x16 1032x16 1028x16 1024x16 1020x16 1016x16 1012x16 1008x16 1004x17 1000x16 "
        "996x16 992x17 988x17 984x16 980x17 976x17 972x17 968x16 964x17 960x18 956x17 952x17 948x17 944x18 "
        "940x17 936x17 932x18 928x18 924x17 920x18 916x18 912x18 908x18 904x18 900x18 896x19 892x18 888x19 "
        "884x18 880x19 876x18 872x19 868x19 864x19 860x19 856x19 852x19 848x20 844x19 840x20 836x19 832x20 "
        "828x20 824x20 820x20 816x20 812x20 808x20 804x20 800x21 796x21 792x20 788x21 784x21 780x21 776x21 "
        "772x21 768x22 764x21 760x22 756x21 752x22 748x22 744x22 740x22 736x22 732x23 728x22 724x23 720x23 "
        "716x22 712x23 708x24 704x23 700x23 696x24 692x24 688x23 684x24 680x24 676x25 672x24 668x25 664x24 "
        "660x25 656x25 652x25 648x25 644x26 640x25 636x26 632x26 628x26 624x26 620x27 616x26 612x27 608x27 "
        "604x27 600x28 596x27 592x28 588x28 584x28 580x28 576x28 572x29 568x29 564x29 560x29 556x30 552x29 "
        "548x30 544x30 540x31 536x30 532x31 528x31 524x31 520x32 516x32 512x32 508x32 504x32 500x33 496x33 "
        "492x33 488x34 484x34 480x34 476x34 472x35 468x35 464x35 460x36 456x36 452x36 448x37 444x37 440x37 "
        "436x37 432x38 428x39 424x38 420x39 416x40 412x39 408x41 404x40 400x41 396x41 392x42 388x42 384x43 "
        "380x43 376x44 372x44 368x44 364x45 360x46 356x46 352x46 348x47 344x48 340x48 336x49 332x49 328x50 "
        "324x51 320x51 316x52 312x52 308x54 304x53 300x55 296x55 292x57 288x56 284x58 280x59 276x59 272x60 "
        "268x61 264x62 260x63 256x64 252x65 248x66 244x68 240x68 236x69 232x71 228x72 224x73 220x74 216x76 "
        "212x77 208x79 204x81 200x81 196x84 192x85 188x88 184x89 180x91 176x93 172x95 168x97 164x100 160x103 "
        "156x105 152x107 148x111 144x114 140x117 136x120 132x124 128x128 124x133 120x136 116x141 112x147 "
        "108x151 104x158 100x164 96x170 92x178 88x186 84x196 80x204 76x216 72x227 68x241 64x256 60x273 56x293 "
        "52x315 48x341 44x373 40x409 36x455 32x512 28x585 24x683 20x819 16x4351 "),
}
for _key, _runs in SCHED_RUNS.items():
    _sizes = [int(r.split("x")[0]) for r in _runs.split() for _ in range(int(r.split("x")[1]))]
    SCHED_BOUNDS[_key] = [0] + np.cumsum(_sizes).tolist()


@pytest.mark.parametrize("key", sorted(SCHED_BOUNDS), ids=lambda k: f"{'stft1024' if k[0] == SCHED_STFT1024 else 'cstft'}-{k[1]}-{k[2]}")
def test_guided_chunks_match_the_recorded_loops(harness, key):
    # guided_sched.h's guided_chunks against the bounds the two launchers' own loops produced
    consts, total, wgs = key
    out = run(harness, "sched", total, wgs, *consts).split()
    assert out[0] == "ok"
    bounds = [int(v) for v in out[1:]]
    assert bounds[0] == 0 and bounds[-1] == total
    assert all(a < b for a, b in zip(bounds, bounds[1:]))
    if consts == SCHED_CSTFT:
        assert all(b % 4 == 0 for b in bounds[:-1])
    assert bounds == SCHED_BOUNDS[key]


@pytest.mark.parametrize("seed", [1, 2])
def test_i8_digits_under_sanitizers(harness, seed):
    # i8_digits.h, the host half of the three int8-MFMA kernels' exactness argument: balanced_digits<6>
    # and <7> reproduce T or refuse it exactly when it does not fit, zero_sum_round's integers sum to 0
    # within 1 of the scaled coefficients, block_i8_coeffs / welch_i8_coeffs (what the plans and
    # msd_i8_coeffs compute) fit seven digits and sum to zero, refine_i8_coeffs (the refinement step's
    # twiddle integers) fit six digits and 2^46 at N 1024 .. 8192, edge and random bins, with cos = 2^46 at
    # n = 0, frag_sample maps a K step's fragment bytes onto its samples
    out = run(harness, "i8", seed, 200000)
    assert out.startswith("ok") and out.split()[3] == "200000", out
