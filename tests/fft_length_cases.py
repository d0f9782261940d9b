"""The case table of tests/test_gpu_fft_lengths.py: every row-transform length, every column length and every entry of the
column kernel table of csrc/fftnative.hip, with the geometry that reaches each -- generated from the length lists by a
plain-Python mirror of `factorize` / `next_length` (csrc/jd_fftcore.h), `column_lanes`, `cols_choice` and `row_schedule`
(csrc/fftnative.hip), and the comparison code of those tests.

tests/test_fft_length_cases_host.py checks, without a GPU, the mirror against the C++ functions for every n up to 9216, the
column table below against the one in the source, and that the generated cases cover what this docstring says.  The GPU
tests assert the route the library reports (`ConvPlan.fft_route`) against the mirror before they trust a number."""
import functools

import numpy as np

ROW_MAX, COLUMN_MAX, COLUMN_TWO_WAVE_MAX = 9216, 4608, 2304  # GENERIC_HUGE, COLUMN_MAX, COLUMN_TWO_WAVE_MAX
GENERIC_TINY, GENERIC_SMALL, GENERIC_LARGE, ROW_MAX_POINTS_LARGE = 1024, 1536, 5120, 4608
MAX_PASSES = 6
N_CU = 256  # compute units of an MI355X (the GPU tests ask the device)
MIN_WIDTH = 8  # fftn_supported: narrower images run on rocFFT
ROW_KWS = (1, 2, 3, 8, 9, 17)  # PSF widths the row cases cycle over: halos 0, 1 (one-sided), 1, 4 (3 | 4), 4, 8
COLS_W, COLS_K = 64, (9, 9)  # the column cases: images 64 columns wide, 9 x 9 PSF (Nx = 72)
FORCED_NY = (512, 576, 1024, 1152, 2048, 2304)  # column lengths with compile-time entries: run with JD_FFT_NATIVE = 2, 4, 8 too
FORCED_CB = (2, 4, 8)

# (lanes, columns per block, radix schedule) of the entries of COLS_TABLE (csrc/fftnative.hip), () = the generic form
COLS_TABLE = (
    (64, 4, (16, 8, 9)), (64, 8, (16, 8, 9)), (128, 2, (16, 16, 9)), (128, 4, (16, 16, 9)), (128, 8, (16, 16, 9)),
    (64, 4, (16, 8, 8)), (128, 2, (16, 16, 8)), (128, 4, (16, 16, 8)), (64, 4, (8, 8, 9)), (64, 4, (8, 8, 8)),
    (64, 0, ()), (256, 0, ()),  # (two-wave columns -- 2048, 2304 -- have compile-time entries only)
)


def cols_max_threads(lanes, cb):
    return 1024 if lanes * cb > 512 else 512


# ---- csrc/jd_fftcore.h ---------------------------------------------------------------------------------------------------
def factorize(N):
    """Radix schedule of N = 2^a * {1, 3, 9}, a >= 3 (tuple; empty: not supported)."""
    m, odd = N, 1
    while m % 3 == 0 and odd < 9:
        m //= 3
        odd *= 3
    if m < 8 or m & (m - 1):
        return ()
    a = m.bit_length() - 1
    n16, n8, n4 = a // 4, 0, 0
    rest = a - 4 * n16
    while rest % 3 != 0 and n16 > 0:
        n16 -= 1
        rest += 4
    if rest % 3 == 0:
        n8 = rest // 3
    elif a == 5:
        n16, n8, n4 = 0, 1, 1
    else:
        return ()
    if n16 + n8 + n4 + (odd > 1) > MAX_PASSES:
        return ()
    return (16,) * n16 + (8,) * n8 + (4,) * n4 + ((odd,) if odd > 1 else ())


def next_length(n, with_three=True):
    """Smallest supported length >= n (0: none); columns keep to 2^a * {1, 9} (with_three = False)."""
    best = 0
    for odd in (1, 3, 9):
        if odd == 3 and not with_three:
            continue
        m = 8
        while m <= 1 << 20:
            v = m * odd
            if v >= n and v >= 32 and factorize(v):
                if not best or v < best:
                    best = v
                break
            m *= 2
    return best


# ---- csrc/fftnative.hip --------------------------------------------------------------------------------------------------
def column_lanes(N):
    f = factorize(N)
    if len(f) < 2 or N > COLUMN_MAX:
        return 0
    choices = (256,) if N > COLUMN_TWO_WAVE_MAX else (64, 128)
    for lanes in choices:
        ok = True
        for R in f:
            per = (N // R + lanes - 1) // lanes
            ok = ok and ((R == 16 and per <= (1 if lanes == 256 else 2)) or (R == 8 and per <= 3) or (R == 9 and per <= 2) or (R == 4 and per <= 2))
        if ok:
            return lanes
    return 0


def lp_size(n):
    return n + (n >> 4) + 1


def _cols_entry(f, lanes, cb):
    for t_lanes, t_cb, t_f in COLS_TABLE:
        if t_lanes == lanes and (not t_f or (t_f == f and t_cb == cb)):
            return t_lanes, t_cb, t_f
    return None


def column_route(Nx, Ny, forced=None):
    """(lanes, columns per block, 1 for a compile-time entry) of the column launch: `cols_choice`.  ``forced``: the value of
    JD_FFT_NATIVE (2 / 4 / 8 force the columns per block where the entry that leads to can be launched)."""
    f, lanes = factorize(Ny), column_lanes(Ny)
    assert lanes, Ny
    two_wave = lanes == 128 and f in ((16, 16, 9), (16, 16, 8))
    cb = 8 if (lanes == 64 and f == (16, 8, 9)) else 4 if (lanes == 64 or two_wave) else 2
    while cb > 2 and Nx % cb:
        cb //= 2
    entry = _cols_entry(f, lanes, cb)
    if forced in (2, 4, 8) and forced * lp_size(Ny) * 8 <= 160 * 1024 and Nx % forced == 0 and (lanes < 256 or forced == 2):
        e = _cols_entry(f, lanes, forced)
        if e and forced * lanes <= cols_max_threads(e[0], e[1]):
            cb, entry = forced, e
    assert cb * lanes <= cols_max_threads(entry[0], entry[1])
    return lanes, cb, 1 if entry[2] else 0


def row_schedule(Nx, W, tiny=False, blocks=0, n_cu=N_CU):
    """Name (ConvPlan.ROW_SCHEDULES) of the row kernels of a launch of ``blocks`` row pairs on a device of ``n_cu`` compute
    units; ``tiny``: option JD_FFT_TINY = 1024 is set."""
    static = {(16, 16, 9): "2304", (8, 8, 8, 9): "4608", (16, 8, 9): "1152"}
    f = factorize(Nx)
    if f in static:
        return static[f]
    if Nx > ROW_MAX_POINTS_LARGE or W > GENERIC_LARGE:
        return "generic-huge"
    if Nx <= GENERIC_TINY and W <= GENERIC_TINY and (tiny or blocks >= 3 * n_cu):  # (one wave per row pair fills the chip)
        return "tiny"
    return "generic-small" if Nx <= GENERIC_SMALL and W <= GENERIC_SMALL else "generic-large"


def geometry(H, W, kh, kw):
    """(Hh, Nx, Ny) of a native plan (fftn_create), None where `fftn_supported` refuses."""
    Hh, ox = (H + 1) // 2, (kw - 1) // 2
    if H < 2 or Hh < kh or W < MIN_WIDTH or W > ROW_MAX:
        return None
    Nx, Ny = next_length(W + max(ox, kw - 1 - ox)), next_length(Hh + kh - 1, False)
    if not (0 < Nx <= ROW_MAX and 0 < Ny <= COLUMN_MAX and Ny >= 2 * kh and column_lanes(Ny)):
        return None
    return Hh, Nx, Ny


ROW_LENGTHS = tuple(n for n in range(32, ROW_MAX + 1) if next_length(n) == n)
COLUMN_LENGTHS = tuple(n for n in range(32, COLUMN_MAX + 1) if next_length(n, False) == n and column_lanes(n))


# ---- the cases -----------------------------------------------------------------------------------------------------------
def _case(kind, H, W, kh, kw, options=()):
    Hh, Nx, Ny = geometry(H, W, kh, kw)
    opts = dict(options)
    tiny = "JD_FFT_TINY" in opts
    lanes, cb, static = column_route(Nx, Ny, opts.get("JD_FFT_NATIVE"))
    name = f"{kind}-{H}x{W}-k{kh}x{kw}" + "".join(f"-{k[3:].lower()}{v}" for k, v in sorted(opts.items()))
    return {"id": name, "kind": kind, "shape": (H, W), "kshape": (kh, kw), "options": opts, "Hh": Hh, "Nx": Nx, "Ny": Ny,
            "tiny": tiny, "rows": row_schedule(Nx, W, tiny, Hh), "cols": (lanes, cb, static)}


def row_widths(Nx, kw, below):
    """The three widths of a row length: full (W + halo == Nx), the ragged neighbour (W % 4 != 0), the smallest width of the
    length (``below``: the next shorter length, 0 for the shortest)."""
    h = kw // 2
    full = Nx - h
    ragged = next(full - d for d in (1, 2, 3) if (full - d) % 4)
    smallest = max(MIN_WIDTH, below + 1 - h)
    assert ragged + h > below and smallest + h > below
    return full, ragged, smallest


def row_cases(tiny=False):
    """A: images of 24 and 25 rows, kh = 5 (Ny = 32), every row length at three widths; ``tiny``: the lengths up to 1024 with
    JD_FFT_TINY = 1024."""
    cases = []
    for i, Nx in enumerate(ROW_LENGTHS):
        if tiny and Nx > GENERIC_TINY:
            continue
        kw = ROW_KWS[i % len(ROW_KWS)]
        below = ROW_LENGTHS[i - 1] if i else 0
        for j, W in enumerate(row_widths(Nx, kw, below)):
            H = 24 if (i + j) % 2 == 0 else 25
            cases.append(_case("rows", H, W, 5, kw, {"JD_FFT_TINY": GENERIC_TINY} if tiny else ()))
            assert cases[-1]["Nx"] == Nx and cases[-1]["Ny"] == 32
    return cases


def column_heights(Ny, kh, below):
    """Exact fit (Hh + kh - 1 == Ny, even H), its odd neighbour, the smallest H of the length."""
    Hh = Ny - kh + 1
    smallest = max(kh, below + 1 - (kh - 1))
    return 2 * Hh, 2 * Hh - 1, 2 * smallest - 1


def column_cases():
    """B: 64 columns, 9 x 9 PSF; every column length at three heights, two short edge cases, the forced columns per block on
    the lengths with compile-time entries, and one square case with Nx = Ny = 1152."""
    kh, kw = COLS_K
    cases = []
    for i, Ny in enumerate(COLUMN_LENGTHS):
        below = COLUMN_LENGTHS[i - 1] if i else 0
        for H in column_heights(Ny, kh, below):
            cases.append(_case("cols", H, COLS_W, kh, kw))
            assert cases[-1]["Ny"] == Ny and cases[-1]["Nx"] == 72
    cases.append(_case("cols-hh-eq-kh", 2 * kh, COLS_W, kh, kw))        # Hh == kh
    cases.append(_case("cols-ny-eq-2kh", 34, COLS_W, 16, kw))           # Ny == 2 kh (and Hh + kh - 1 == Ny)
    assert cases[-2]["Hh"] == kh and cases[-1]["Ny"] == 2 * 16
    for Ny in FORCED_NY:
        for cb in FORCED_CB:
            cases.append(_case("cols-forced", 2 * (Ny - kh + 1), COLS_W, kh, kw, {"JD_FFT_NATIVE": cb}))
            assert cases[-1]["Ny"] == Ny
    cases.append(_case("cols-square", 2 * (1152 - kh + 1), 1152 - kw // 2, kh, kw))
    assert (cases[-1]["Nx"], cases[-1]["Ny"], cases[-1]["cols"]) == (1152, 1152, (64, 8, 1))
    return cases


# C: (H, W) of the un-up-sampled likelihood step with a 5 x 7 PSF, and whether JD_FFT_TINY = 1024 is set: one shape per row
# schedule, and a power-of-two length for each generic class
STEP_SHAPES = (
    ((24, 139), False), ((25, 250), False),     # generic-small: 144 = 16 9, 256 = 16 16
    ((24, 3000), False), ((25, 4090), False),   # generic-large: 3072 = 16 8 8 3, 4096 = 16 16 16
    ((24, 6000), False), ((25, 8180), False),   # generic-huge: 6144, 8192
    ((24, 1148), False), ((25, 2300), False), ((24, 4600), False),  # the compile-time schedules 1152, 2304, 4608
    ((24, 90), True), ((25, 60), True),         # tiny: 96 = 8 4 3, 64 = 8 8
)
STEP_K = (5, 7)


def step_cases():
    return [_case("step", H, W, *STEP_K, {"JD_FFT_TINY": GENERIC_TINY} if tiny else ()) for (H, W), tiny in STEP_SHAPES]


# D: a power-of-two row length, an odd H, an exact-fit column; PSF 9 x 13
IMPULSE_K = (9, 13)
IMPULSE_SHAPES = ((40, 58), (41, 100), (48, 60))


def impulse_cases():
    cases = [_case("impulse", H, W, *IMPULSE_K) for H, W in IMPULSE_SHAPES]
    assert cases[0]["Nx"] == 64 and cases[2]["Hh"] + IMPULSE_K[0] - 1 == cases[2]["Ny"]
    return cases


def all_cases():
    return row_cases() + row_cases(tiny=True) + column_cases() + step_cases() + impulse_cases()


# ---- inputs, references and the comparison -------------------------------------------------------------------------------
def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def general_psf(kshape, seed=7):
    rs = np.random.RandomState(seed)
    psf = rs.uniform(0.0, 1.0, size=kshape) ** 3  # a general (full-rank) kernel
    return (psf / psf.sum()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def conv_inputs(shape):
    """image, scale image, a second image for the adjoint identity: the inputs of tests/test_gpu_fft_native.py"""
    H, W = shape
    rs = np.random.RandomState(H + W)
    image = rs.gamma(2.0, size=shape).astype(np.float32)
    image[rs.randint(0, H, 20), rs.randint(0, W, 20)] += 500.0  # point sources: a large dynamic range
    scale = rs.uniform(0.5, 1.5, size=shape).astype(np.float32)
    y = rs.uniform(size=shape).astype(np.float32)
    for a in (image, scale, y):
        a.setflags(write=False)
    return image, scale, y


def conv_references(image, scale, psf):
    """float64: conv_same(image * scale, psf) and its transpose scale * corr_same(image, psf)"""
    from scipy.signal import fftconvolve

    (H, W), (kh, kw) = image.shape, psf.shape
    oy, ox = (kh - 1) // 2, (kw - 1) // 2
    full = fftconvolve(image.astype(np.float64) * scale, psf.astype(np.float64), mode="full")
    full_adj = fftconvolve(image.astype(np.float64), psf[::-1, ::-1].astype(np.float64), mode="full")
    ay, ax = kh - 1 - oy, kw - 1 - ox
    return full[oy:oy + H, ox:ox + W], full_adj[ay:ay + H, ax:ax + W] * scale


def error_bound(e_roc):
    """The rule of tests/test_gpu_fft_wide.py: the library's 2e-6, or twice the error of the rocFFT plan on the same inputs"""
    return max(2e-6, 2.0 * e_roc)


def within_bound(got, want, e_roc):
    """(passes, relative L-inf error of `got` against the float64 `want`)"""
    e = rel_linf(got, want)
    return e <= error_bound(e_roc), e


def impulse_psf():
    kh, kw = IMPULSE_K
    return (1.0 + np.arange(kh * kw, dtype=np.float32)).reshape(kh, kw)  # distinct taps 1 + index


def impulse_positions(H, W):
    """The four corners, rows Hh - 1 and Hh (the seam between the two image rows of one complex transform), the last column"""
    Hh = (H + 1) // 2
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (Hh - 1, W // 3), (Hh, (2 * W) // 3), (H // 4, W - 1)]


def impulse_image(H, W):
    image = np.zeros((H, W), dtype=np.float32)
    for y, x in impulse_positions(H, W):
        image[y, x] = 1.0
    return image


def impulse_reference(H, W, psf, adjoint=False):
    """float64 placement of the PSF (its transpose: mirrored about the origin tap) at every impulse, and the mask of the
    pixels inside a footprint"""
    kh, kw = psf.shape
    oy, ox = (kh - 1) // 2, (kw - 1) // 2
    ref, inside = np.zeros((H, W)), np.zeros((H, W), dtype=bool)
    for y, x in impulse_positions(H, W):
        for a in range(kh):
            for b in range(kw):
                yy, xx = (y - (a - oy), x - (b - ox)) if adjoint else (y + a - oy, x + b - ox)
                if 0 <= yy < H and 0 <= xx < W:
                    ref[yy, xx] += float(psf[a, b])
                    inside[yy, xx] = True
    return ref, inside


def impulse_failures(got, ref, inside, max_tap):
    """Violations of D: every pixel within 2e-6 x the largest tap of the placement; away from the footprints the result below
    that bound in absolute terms"""
    got = np.asarray(got, dtype=np.float64)
    bound = 2e-6 * max_tap
    failures = []
    e_in = np.abs(got - ref)[inside].max()
    e_out = np.abs(got[~inside]).max() if (~inside).any() else 0.0
    if not e_in <= bound:
        y, x = np.unravel_index(np.argmax(np.where(inside, np.abs(got - ref), -1.0)), got.shape)
        failures.append(f"footprints: {e_in:.3e} > {bound:.3e} at ({y}, {x})")
    if not e_out <= bound:
        y, x = np.unravel_index(np.argmax(np.where(inside, -1.0, np.abs(got))), got.shape)
        failures.append(f"outside the footprints: {e_out:.3e} > {bound:.3e} at ({y}, {x})")
    return failures, e_in, e_out
