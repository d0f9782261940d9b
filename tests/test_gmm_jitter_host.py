"""CPU: the index arithmetic of the jittered patch grid (csrc/jd_jitter.h: grid count, safety, clamped positions, the
candidate window of a pixel and its cover list) compiled for the host (tests/native/jitter_check.cpp) and run, for every
case and every extreme draw of tests/gmm_jitter_cases.py, against numpy's brute force."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gmm_jitter_cases as cases

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    out = tmp_path_factory.mktemp("jitter") / "jitter_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", str(REPO / "jolideco_amd" / "csrc"),
                    str(REPO / "tests" / "native" / "jitter_check.cpp"), "-o", str(out)], check=True)
    return out


def _axes():
    """[(label, n, P, s, roll, draws)]: both axes of every case and of every extreme draw, plus draws beyond the range"""
    axes = []
    for table in (64, 256):
        rows, patch, _ = cases.table_of(table)
        for index, (shape, stride, roll) in enumerate(rows):
            jitter = cases.case_draws(index, table)
            for axis in (0, 1):
                axes.append((f"D = {table} case {index} axis {axis}", shape[axis], patch, stride, 0 if roll is None else roll[axis], jitter[axis]))
    for name, jitter in cases.extreme_draws().items():
        for axis in (0, 1):
            axes.append((f"extreme {name} axis {axis}", (40, 44)[axis], 8, 4, (2, -1)[axis], jitter[axis]))
    axes.append(("beyond the range", 40, 8, 4, 3, np.array([9, -9, 5, -5, 100, -100, 0])))
    # (strides below half a patch are never safe -- the entry refuses them -- but the window arithmetic holds for them too)
    axes.append(("stride 1", 40, 8, 1, -2, np.random.RandomState(1).randint(-7, 8, size=len(cases.grid((40, 40), 8, 1)[0]))))
    axes.append(("stride 1, 16 x 16", 64, 16, 1, 5, np.random.RandomState(2).randint(-15, 16, size=len(cases.grid((64, 64), 16, 1)[0]))))
    return axes


def test_window_and_cover_lists_equal_brute_force(exe):
    axes = _axes()
    text = "".join(f"{n} {P} {s} {roll} {len(d)} {' '.join(str(int(v)) for v in d)}\n" for _, n, P, s, roll, d in axes)
    done = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    lines = iter(done.stdout.splitlines())
    checked = longest = 0
    for label, n, P, s, roll, draws in axes:
        head = next(lines).split()
        overlap = P - s
        assert head[0] == "axis" and [int(v) for v in head[1:4]] == [n, P, s], label
        count, safe, maxc = (int(v) for v in head[4:])
        assert count == len(draws) == len(np.arange(overlap, n - s - overlap, s)), label
        assert safe == int(cases.is_safe((n, n), P, s)) == int(s >= 4) and maxc == (2 * overlap + P - 1) // s + 1, label
        clamped = np.clip(draws, -overlap, overlap)  # (the header clamps a draw: the kernels cannot validate one)
        brute = cases.cover_lists(n, P, s, clamped, roll)
        for p in range(n):
            row = [int(v) for v in next(lines).split()]
            assert row[0] == p and row[1] == (p + roll) % n and row[4] == len(row) - 5 <= maxc, (label, p)
            lo, hi = row[2], row[3]
            pairs = [divmod(v, P) for v in row[5:]]
            assert pairs == brute[p], (label, p, pairs, brute[p])
            assert all(lo <= i <= hi for i, _ in brute[p]) and hi - lo + 1 <= maxc and 0 <= lo and hi < count, (label, p, lo, hi)
            checked += 1
            longest = max(longest, len(pairs))
    assert next(lines, None) is None and checked == sum(a[1] for a in axes) and longest >= 16


def test_count_and_safety_of_the_issue_lengths(exe):
    """P = 8, s = 4: 40, 44, 72, 100 are safe, 37, 41, 27 are not; P = 16, s = 8: 48, 56 are safe, 44 is not; a length without
    a patch is not safe"""
    table = [(n, 8, 4, True) for n in (40, 44, 72, 100)] + [(n, 8, 4, False) for n in (37, 41, 27, 12, 8)]
    table += [(48, 16, 8, True), (56, 16, 8, True), (44, 16, 8, False), (24, 8, 8, True), (27, 8, 8, True)]
    done = subprocess.run([str(exe)], input="".join(f"{n} {P} {s} 0 -1\n" for n, P, s, _ in table), capture_output=True, text=True)
    assert done.returncode == 0
    lines = done.stdout.splitlines()
    assert len(lines) == len(table)
    for line, (n, P, s, safe) in zip(lines, table):
        head = [int(v) for v in line.split()[1:]]
        assert head[:3] == [n, P, s] and head[3] == len(cases.grid((n, n), P, s)[0]) and head[4] == int(safe), line
        assert cases.is_safe((n, n), P, s) == safe
