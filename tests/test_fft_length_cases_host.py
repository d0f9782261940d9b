"""CPU: the case table of tests/test_gpu_fft_lengths.py (tests/fft_length_cases.py).

1. Its plain-Python mirror of `factorize` / `next_length` agrees with csrc/jd_fftcore.h for every n up to 9216
   (tests/native/fft_lengths_dump.cpp, built with g++), and its column table is the one in csrc/fftnative.hip.
2. The generated cases contain every row length and every column length, every row length up to 1024 a second time on the
   one-wave kernels, every entry of the column table, and the geometric edges -- "every length" is a checked property.
3. The comparison code rejects a reference that is shifted by one row, by one column, or lacks one PSF tap: the bound of the
   convolution cases for every tap large enough to rise above it under a point source, the impulse check for the smallest of its taps too."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fft_length_cases as flc

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "jolideco_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_mirror_agrees_with_the_header_for_every_length(tmp_path):
    exe = tmp_path / "fft_lengths_dump"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", str(CSRC), str(REPO / "tests" / "native" / "fft_lengths_dump.cpp"), "-o", str(exe)],
                   check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    lines = done.stdout.splitlines()
    assert len(lines) == flc.ROW_MAX
    for line in lines:
        head, radices = line.split(":")
        n, rows, cols = (int(v) for v in head.split())
        assert flc.next_length(n) == rows and flc.next_length(n, False) == cols, line
        assert flc.factorize(n) == tuple(int(v) for v in radices.split()), line


def test_the_column_table_is_the_one_in_the_source():
    text = (CSRC / "fftnative.hip").read_text()
    entries = re.findall(r"^\s*JD_COLS_ENTRY\((\d+), (\d+), (\d+), (\d+), (\d+)\)", text, flags=re.M)
    table = tuple((int(e[0]), int(e[1]), tuple(int(v) for v in e[2:]) if int(e[2]) else ()) for e in entries)
    assert len(table) == 12 and table == flc.COLS_TABLE
    # the limit of an entry is its kernel's launch bound: one expression for both
    assert "__launch_bounds__((cols_max_threads(LANES, CBS))" in text
    assert "fftn_cols_kernel<L, CB, R0, R1, R2>, cols_max_threads(L, CB)}" in text
    assert re.search(r"constexpr int cols_max_threads\(int LANES, int CBS\) \{ return LANES \* CBS > 512 \? 1024 : 512; \}", text)
    # and one function chooses for the launch and for the query
    assert len(re.findall(r"= cols_choice\(n\)", text)) == 2


def test_the_length_lists():
    assert len(flc.ROW_LENGTHS) == 25 and len(flc.COLUMN_LENGTHS) == 15
    assert flc.ROW_LENGTHS[0] == 32 and flc.ROW_LENGTHS[-1] == 9216 and flc.COLUMN_LENGTHS[-1] == 4608
    assert set(flc.COLUMN_LENGTHS) == {n for n in flc.ROW_LENGTHS if n % 3 or n % 9 == 0} - {n for n in flc.ROW_LENGTHS if n > 4608}
    assert sum(1 for n in flc.ROW_LENGTHS if n <= 1024) == 15


def test_every_length_and_every_table_entry_has_a_case():
    rows, tiny, cols = flc.row_cases(), flc.row_cases(tiny=True), flc.column_cases()
    # every row length, at three widths: full (W + halo == Nx), ragged, smallest
    for Nx in flc.ROW_LENGTHS:
        mine = [c for c in rows if c["Nx"] == Nx]
        assert len(mine) == 3 and len({c["shape"][1] for c in mine}) == 3, Nx
        halo = mine[0]["kshape"][1] // 2
        assert mine[0]["shape"][1] + halo == Nx and mine[1]["shape"][1] % 4 != 0
        assert flc.geometry(mine[2]["shape"][0], mine[2]["shape"][1] - 1, *mine[2]["kshape"]) is None or \
            flc.geometry(mine[2]["shape"][0], mine[2]["shape"][1] - 1, *mine[2]["kshape"])[1] < Nx
        want = (str(Nx) if Nx in (1152, 2304, 4608) else "generic-small" if Nx <= 1536 else
                "generic-large" if Nx in (2048, 3072, 4096) else "generic-huge")
        assert {c["rows"] for c in mine} == {want}, Nx
        # ... and up to 1024 a second time on the one-wave kernels
        again = [c for c in tiny if c["Nx"] == Nx]
        assert (len(again) == 3 and {c["rows"] for c in again} == {"tiny"}) if Nx <= 1024 else not again, Nx
    assert {c["shape"][0] for c in rows} == {24, 25} and {c["Ny"] for c in rows} == {32}
    assert {c["kshape"][1] for c in rows} == set(flc.ROW_KWS)
    # no padding column at all: kw = 1 and W == Nx (among them the longest row)
    assert any(c["kshape"][1] == 1 and c["shape"][1] == c["Nx"] == 9216 for c in rows)
    # every column length: exact fit with an even H, its odd neighbour, the smallest H
    for Ny in flc.COLUMN_LENGTHS:
        mine = [c for c in cols if c["kind"] == "cols" and c["Ny"] == Ny]
        assert len(mine) == 3, Ny
        assert mine[0]["Hh"] + 9 - 1 == Ny and mine[0]["shape"][0] % 2 == 0 and mine[1]["shape"][0] == mine[0]["shape"][0] - 1
        assert mine[2]["shape"][0] % 2 == 1
        smaller = flc.geometry(mine[2]["shape"][0] - 2, flc.COLS_W, 9, 9)
        assert smaller is None or smaller[2] < Ny
        assert {c["cols"][0] for c in mine} == {64 if Ny <= 1152 else 128 if Ny <= 2304 else 256}
    assert any(c["Hh"] == c["kshape"][0] for c in cols) and any(c["Ny"] == 2 * c["kshape"][0] for c in cols)
    # every entry of the column table is the route of some case
    reached = set()
    for c in cols:
        lanes, cb, static = c["cols"]
        reached.add((lanes, cb, flc.factorize(c["Ny"])) if static else (lanes, 0, ()))
    assert reached == set(flc.COLS_TABLE)
    # the generic kernels on the lengths with a compile-time entry
    assert {(c["Ny"], c["cols"]) for c in cols if c["kind"] == "cols-forced" and not c["cols"][2]} >= {
        (512, (64, 2, 0)), (512, (64, 8, 0)), (576, (64, 2, 0)), (576, (64, 8, 0)), (1024, (64, 2, 0)), (1024, (64, 8, 0)), (1152, (64, 2, 0))}
    ids = [c["id"] for c in flc.all_cases()]
    assert len(ids) == len(set(ids))


def test_a_forced_block_never_exceeds_the_launch_bounds_of_its_entry():
    """Ny = 2048 with JD_FFT_NATIVE = 8: no {128, 8, 16, 16, 8} entry, and the generic two-wave kernel is compiled for 512
    threads -- the default (four columns, compile-time entry) stands."""
    assert flc.column_route(72, 2048, forced=8) == (128, 4, 1)
    assert flc.column_route(72, 2304, forced=8) == (128, 8, 1)  # (this one has its entry, compiled for 1024 threads)
    for Ny in flc.COLUMN_LENGTHS:
        for Nx in (72, 1152, 9216):
            for forced in (None, 2, 4, 8):
                lanes, cb, static = flc.column_route(Nx, Ny, forced)
                assert lanes * cb <= (1024 if static else 512) and Nx % cb == 0


def test_the_library_takes_every_case():
    from jolideco_amd import _hip

    lib = _hip.lib()
    for c in flc.all_cases():
        assert lib.jd_conv_native_fft_supported(*c["shape"], *c["kshape"]) == 1, c["id"]


# ---- E: the comparison code proves itself ---------------------------------------------------------------------------------
def _fp32_convolution(image, scale, psf):
    """A correct single-precision FFT convolution (scipy's, on float32 arrays): stands for a kernel's result"""
    from scipy.signal import fftconvolve

    (H, W), (kh, kw) = image.shape, psf.shape
    oy, ox = (kh - 1) // 2, (kw - 1) // 2
    full = fftconvolve(image * scale, psf, mode="full")
    assert full.dtype == np.float32
    return full[oy:oy + H, ox:ox + W]


@pytest.mark.parametrize("shape,kshape", [((24, 61), (5, 3)), ((25, 247), (5, 17))])
def test_the_bound_of_the_convolution_cases_rejects_a_wrong_reference(shape, kshape):
    image, scale, _ = flc.conv_inputs(shape)
    psf = flc.general_psf(kshape)
    ref, _ = flc.conv_references(image, scale, psf)
    got = _fp32_convolution(image, scale, psf)
    e_roc = flc.rel_linf(got, ref)  # (the error a second single-precision implementation would show)
    ok, e = flc.within_bound(got, ref, e_roc)
    assert ok and e < 2e-6, e
    wrong = {"one row down": np.roll(ref, 1, axis=0), "one column right": np.roll(ref, 1, axis=1)}
    for name, want in wrong.items():
        ok, e = flc.within_bound(got, want, e_roc)
        print(f"{name}: {e:.2e} against a bound of {flc.error_bound(e_roc):.2e}")
        assert not ok, name
    # One tap dropped, every tap in turn.  A point source (+500, scale >= 0.5) puts >= 250 x the tap into one pixel, so the
    # bound must see every tap above bound x max|ref| / 250; the taps of this u^3 kernel below that (a few of the smallest)
    # are what the impulse check with its taps 1 .. 117 is for.
    visible = flc.error_bound(e_roc) * np.abs(ref).max() / 250.0
    seen = 0
    for index in np.ndindex(*psf.shape):
        dropped = psf.copy()
        dropped[index] = 0.0
        ok, e = flc.within_bound(got, flc.conv_references(image, scale, dropped)[0], e_roc)
        if psf[index] > visible:
            assert not ok, (index, float(psf[index]), e)
            seen += 1
    print(f"a dropped tap is rejected for {seen} of {psf.size} taps (those above {visible:.2e}; largest tap {psf.max():.2e})")
    assert seen >= 0.9 * psf.size


@pytest.mark.parametrize("H,W", flc.IMPULSE_SHAPES)
def test_the_impulse_check_rejects_a_wrong_result(H, W):
    psf = flc.impulse_psf()
    for adjoint in (False, True):
        ref, inside = flc.impulse_reference(H, W, psf, adjoint)
        # the placement is the convolution
        conv, adj = flc.conv_references(flc.impulse_image(H, W), np.ones((H, W), dtype=np.float32), psf)
        assert np.abs((adj if adjoint else conv) - ref).max() < 1e-9
        assert 0.1 < inside.mean() < 0.9
        good = ref.astype(np.float32)
        assert flc.impulse_failures(good, ref, inside, psf.max())[0] == []
        dropped = psf.copy()
        dropped[0, 0] = 0.0  # the smallest tap: 1 of 1 .. 117
        mirrored = psf[::-1, ::-1]
        wrong = {"one row down": np.roll(good, 1, axis=0), "one column right": np.roll(good, 1, axis=1),
                 "the smallest tap dropped": flc.impulse_reference(H, W, dropped, adjoint)[0],
                 "mirrored taps": flc.impulse_reference(H, W, mirrored, adjoint)[0],
                 "leakage across the seam": good + 1e-3 * np.roll(good, H // 2, axis=0)}
        for name, got in wrong.items():
            assert flc.impulse_failures(got, ref, inside, psf.max())[0], name
