"""NumPy models of the correction of raw detector movies (csrc/moviefix.hip, include/sprk.h: sprk_movie_correct,
spr_pick_amd/moviefix.py), the oracle of tests/test_moviefix_cpu.py and tests/test_gpu_moviefix.py.

The device contract, per pixel p = (y, x) with d the sample as float32:
  c(p) = d; with dark c = d - dark[p]; with gain c = c * gain[p]: one float32 rounding each, nothing fused;
  fix[p] == 0:      out[p] = c(p);
  fix[p] == r > 0:  r = min(r, 8); over the window clamped to the frame, row-major, over the q with fix[q] == 0:
                    S = S + c(q) in float32 from 0, n their count; out[p] = S / n in float32, or 0 when n == 0;
  the sum:          one float32 chain per pixel over the frames in call order.
The window, ``build_fix`` and ``detect_hot`` are plain loops here; the package builds the map by max-pooling."""
import numpy as np

FIX_MAX_RADIUS = 8


def corrected(raw, gain=None, dark=None):
    """[ny, nx] samples of any MRC sample type -> c float32, for every pixel, bad ones included"""
    c = np.asarray(raw).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if dark is not None:
            c = (c - dark.astype(np.float32)).astype(np.float32)
        if gain is not None:
            c = (c * gain.astype(np.float32)).astype(np.float32)
    return c


def movie_correct(raw, gain=None, dark=None, fix=None):
    """-> out float32 [ny, nx]"""
    c = corrected(raw, gain, dark)
    if fix is None:
        return c
    ny, nx = c.shape
    assert fix.shape == c.shape and fix.dtype == np.uint8
    out = c.copy()
    for y, x in np.argwhere(fix > 0):
        r = min(int(fix[y, x]), FIX_MAX_RADIUS)
        S, n = np.float32(0.0), 0
        for yy in range(max(0, y - r), min(ny - 1, y + r) + 1):
            for xx in range(max(0, x - r), min(nx - 1, x + r) + 1):
                if fix[yy, xx] == 0:
                    S = np.float32(S + c[yy, xx])
                    n += 1
        out[y, x] = np.float32(S) / np.float32(n) if n else np.float32(0.0)
    return out


def movie_sum(frames, gain=None, dark=None, fix=None):
    """-> (the corrected frames float32 [Z, ny, nx], their sum float32 [ny, nx]: one chain per pixel, frame 0 first)"""
    outs = [movie_correct(f, gain, dark, fix) for f in frames]
    total = outs[0].copy()
    for o in outs[1:]:
        total = (total + o).astype(np.float32)
    return np.stack(outs), total


def static_bad(gain, defects):
    """bool [ny, nx]: the gain is not finite or not positive, or a defect rectangle covers the pixel"""
    bad = np.zeros(defects.shape if gain is None else gain.shape, dtype=bool) if defects is None else defects.copy()
    if gain is not None:
        with np.errstate(invalid="ignore"):
            bad |= ~np.isfinite(gain) | ~(gain > 0)
    return bad


def defect_mask(rects, ny, nx):
    """rects: (x, y, w, h) with x the column and y the row of the first sample -> bool [ny, nx]"""
    m = np.zeros((ny, nx), dtype=bool)
    for x, y, w, h in rects:
        assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= nx and y + h <= ny
        m[y:y + h, x:x + w] = True
    return m


def build_fix(bad):
    """bool [ny, nx] -> uint8: 0 where good, else the smallest r in 1 .. 8 whose window, clamped to the frame, holds a good
    pixel; ValueError when a bad pixel has none within 8"""
    ny, nx = bad.shape
    fix = np.zeros((ny, nx), dtype=np.uint8)
    lost = []
    for y, x in np.argwhere(bad):
        for r in range(1, FIX_MAX_RADIUS + 1):
            if not bad[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].all():
                fix[y, x] = r
                break
        else:
            lost.append((int(y), int(x)))
    if lost:
        raise ValueError("%d bad pixel(s) without a good one within %d, the first at row %d, column %d"
                         % (len(lost), FIX_MAX_RADIUS, lost[0][0], lost[0][1]))
    return fix


def detect_hot(T, bad, sigma, rounds=4):
    """T [ny, nx] (a sum of corrected frames), bad bool -> (bad with the hot pixels added, the thresholds of every round that
    ran): per round mu and the population sigma of the not-bad pixels in float64, new = not bad and T > mu + sigma * std; it
    stops after a round that finds nothing, and after ``rounds``"""
    T = np.asarray(T, dtype=np.float64)
    bad = bad.copy()
    thresholds = []
    for _ in range(rounds):
        vals = []
        for y in range(T.shape[0]):
            for x in range(T.shape[1]):
                if not bad[y, x]:
                    vals.append(T[y, x])
        vals = np.array(vals, dtype=np.float64)
        mu = vals.sum() / len(vals)
        sd = np.sqrt(((vals - mu) ** 2).sum() / len(vals))
        thresholds.append((mu + sigma * sd, sd))
        new = ~bad & (T > mu + sigma * sd)
        if not new.any():
            break
        bad |= new
    return bad, thresholds


# ---- a spoiled movie: what a detector writes for align_model.make_movie's frames -------------------------------------------------
HOT_VALUE, HOT_COUNT = 30000, 40


def spoil(movie, seed, defects=True):
    """movie int16 [Z, ny, nx] (clean, gain-corrected: M) -> dict: gain drawn from {1, 1/2, 1/4}, dark integers in 0 .. 49,
    raw = M / gain + dark as int16 (exact: M < 4096 here), and with ``defects`` one gain column set to 0, one defect rectangle
    (x, y, w, h) whose samples are a stuck value, and HOT_COUNT hot pixels at HOT_VALUE in every frame"""
    Z, ny, nx = movie.shape
    rng = np.random.RandomState(3000 + seed)
    gain = rng.choice(np.array([1.0, 0.5, 0.25], dtype=np.float32), size=(ny, nx))
    dark = rng.randint(0, 50, size=(ny, nx)).astype(np.float32)
    wide = movie.astype(np.int64) * np.rint(1.0 / gain).astype(np.int64) + dark.astype(np.int64)
    assert wide.max() < 32767 and wide.min() > -32768
    raw = wide.astype(np.int16)
    assert np.array_equal(np.stack([corrected(f, gain, dark) for f in raw]), movie.astype(np.float32))
    out = {"gain": gain, "dark": dark, "raw": raw, "rects": [], "hot": np.zeros((ny, nx), dtype=bool), "column": None}
    if not defects:
        return out
    column = int(rng.randint(10, nx - 10))
    gain[:, column] = 0.0
    raw[:, :, column] = 1234                                     # a dead column reads a constant
    rect = (int(rng.randint(20, nx - 40)), int(rng.randint(20, ny - 40)), 6, 4)
    x, y, w, h = rect
    raw[:, y:y + h, x:x + w] = 20000
    covered = defect_mask([rect], ny, nx)
    covered[:, column] = True
    hot = np.zeros((ny, nx), dtype=bool)
    while hot.sum() < HOT_COUNT:
        yy, xx = int(rng.randint(0, ny)), int(rng.randint(0, nx))
        if not covered[yy, xx]:
            hot[yy, xx] = True
    raw[:, hot] = HOT_VALUE
    out.update(rects=[rect], hot=hot, column=column)
    return out


def write_defects(path, rects):
    with open(path, "w") as f:
        f.write("# x y w h\n\n" + "".join("%d %d %d %d\n" % r for r in rects))


def prepare(frames, gain=None, dark=None, defects=None, hot_sigma=None):
    """what spr_pick_amd.moviefix.prepare does, by the loops above -> (static bad, all bad, the fix map, the corrected
    frames float32 [Z, ny, nx])"""
    ny, nx = frames[0].shape
    static = static_bad(gain, np.zeros((ny, nx), dtype=bool) if defects is None else defects)
    bad = static
    if hot_sigma is not None:
        _, total = movie_sum(frames, gain, dark, build_fix(static))
        bad, _ = detect_hot(total, static, hot_sigma)
    fix = build_fix(bad)
    return static, bad, fix, np.stack([movie_correct(f, gain, dark, fix) for f in frames])


# ---- the bad-pixel layouts of both test files, on a 40 x 48 frame ------------------------------------------------------------
FIX_SHAPE = (40, 48)


def fix_cases():
    """-> [(name, bad bool [40, 48], the largest radius its map holds, or None where build_fix must raise)]"""
    ny, nx = FIX_SHAPE

    def blank():
        return np.zeros((ny, nx), dtype=bool)
    cases = []
    b = blank(); b[17, 23] = True
    cases.append(("isolated", b, 1))
    b = blank(); b[0, 0] = b[0, nx - 1] = b[ny - 1, 0] = b[ny - 1, nx - 1] = True
    cases.append(("corners", b, 1))
    b = blank(); b[:, 31] = True
    cases.append(("column", b, 1))
    b = blank(); b[12, :] = True
    cases.append(("row", b, 1))
    b = blank(); b[10:15, 20:25] = True
    cases.append(("blob5", b, 3))
    b = blank(); b[8, 40] = b[8, 41] = True
    cases.append(("pair", b, 1))
    b = blank(); b[12:27, 16:31] = True                          # 15 x 15: the centre is 8 from the nearest good pixel
    cases.append(("blob15", b, 8))
    b = blank(); b[11:28, 15:32] = True                          # 17 x 17: the centre's window of +-8 is the blob itself
    cases.append(("blob17", b, None))
    b = blank(); b[11:30, 15:34] = True
    cases.append(("blob19", b, None))
    return cases
