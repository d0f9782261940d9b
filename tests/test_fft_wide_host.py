"""CPU: the native FFT convolution on images up to 9216 columns x 2 * 4608 rows (csrc/fftnative.hip: the 768-thread
"generic-huge" row kernels, four waves per column) -- which geometries `jd_conv_native_fft_supported` accepts, and the
radix schedules and padded lengths of those sizes on the host against a float64 DFT (tests/native/fftcore_wide_check.cpp),
once more under the address and undefined-behaviour sanitizers."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent

# (image shape, PSF shape) of tests/test_gpu_fft_wide.py: rows beyond 4608 points, columns beyond 2304, both
WIDE = [((24, 4800), (5, 5)), ((66, 6100), (33, 17)), ((26, 8000), (9, 9)), ((34, 8192), (17, 17)), ((25, 9203), (5, 7)),
        ((4700, 64), (9, 9)), ((8192, 64), (17, 17)), ((8001, 68), (9, 5)), ((9000, 64), (9, 9)), ((4700, 4800), (9, 9)),
        # flux grids of the likelihood-step cases and the joint fit
        ((48, 5200), (10, 10)), ((48, 8192), (10, 10)), ((72, 5400), (15, 15)), ((96, 8192), (20, 20)), ((48, 5202), (10, 10)),
        ((4800, 64), (10, 10)), ((16, 5000), (5, 5)), ((16, 5000), (7, 7)),
        # the benchmark's geometries (tools/fft_wide_bench.py)
        ((8192, 8192), (17, 17)), ((8192, 8192), (65, 65)), ((4096, 8192), (17, 17)), ((6000, 6000), (17, 17)), ((8192, 512), (17, 17))]
REFUSED = [((24, 9300), (5, 5)),    # W = 9300 > 9216
           ((24, 9216), (5, 5)),    # 9216 pixels + 2 of the PSF's halo: no length left
           ((9300, 64), (9, 9)),    # Hh + kh - 1 = 4658 > 4608
           ((9216, 64), (9, 9)),    # 4608 + 8
           ((64, 7), (3, 3)), ((9000, 4), (9, 9)),  # W < 8
           ((24, 6100), (33, 17)), ((24, 8192), (17, 17))]  # an image half shorter than the PSF (as at every width)


def test_support_table():
    from jolideco_amd import _hip

    lib = _hip.lib()
    for (H, W), (kh, kw) in WIDE:
        assert lib.jd_conv_native_fft_supported(H, W, kh, kw) == 1, (H, W, kh, kw)
    for (H, W), (kh, kw) in REFUSED:
        assert lib.jd_conv_native_fft_supported(H, W, kh, kw) == 0, (H, W, kh, kw)
    from test_gpu_fft_native import CASES

    for (H, W), (kh, kw) in CASES:  # every geometry of the sizes supported before
        assert lib.jd_conv_native_fft_supported(H, W, kh, kw) == 1, (H, W, kh, kw)


def test_row_schedule_names_keep_their_indices():
    from jolideco_amd.ops import ConvPlan

    assert ConvPlan.ROW_SCHEDULES[:6] == ("generic-large", "2304", "4608", "1152", "generic-small", "tiny")
    assert ConvPlan.ROW_SCHEDULES[6] == "generic-huge" and len(ConvPlan.ROW_SCHEDULES) == 7


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_fft_core_of_the_wide_lengths_matches_a_float64_dft(tmp_path, sanitize):
    exe = tmp_path / "fftcore_wide_check"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", *flags, "-std=c++17", "-I", str(REPO / "jolideco_amd" / "csrc"),
                    str(REPO / "tests" / "native" / "fftcore_wide_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout + done.stderr)[-3000:]
    assert "BAD" not in done.stdout and done.stdout.count("rel err") == 10
    assert "N  9216 dir -1 passes 16 8 8 9" in done.stdout and "N  8192 dir +1 passes 16 8 8 8" in done.stdout
    for line in ("rows: 4802 -> 6144", "rows: 8004 -> 8192", "rows: 8200 -> 9216", "columns: 2358 -> 4096", "columns: 4112 -> 4608"):
        assert line in done.stdout
