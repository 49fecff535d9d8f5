"""Geometry-coverage designs (a helper module of tests/test_geometry_coverage*.py and tests/test_tilewalk_gpu.py, not a conftest).

Where tests/operand_designs.py enumerates the VALUES the per-pixel code meets, this module enumerates the SHAPES the ragged-tile
code meets: every column remainder `cols = W - X0` (1 ... 127) and row remainder `rows = H - Y0` (1 ... TH - 1) of a 128 x TH
tile, with and without an interior neighbour, and the frames that move the corners of the deep levels across the frame's edge.
Everything here is defined from the shapes and from oracle/hgi_numpy.py, never from the library:

1. the shape sets R1, R0 (remainders), D (deep levels) and WALK (the uniform kernels' tile walk), and their seeded content --
   noise in [8, 255], so that no pixel is 0: under the Crossed predictor a corner that turns from 0 (the out-of-image value)
   into 8 or more, or back, always moves the prediction;
2. `tile_classes`: the class of every ragged tile of a shape, from the shape alone;
3. `encode_oob` / `decode_oob`: oracle/hgi_numpy.py with the out-of-image rule of its corner lattice made explicit, five mutants
   of that rule, and `applies`: the exact set of (shape, levels) on which a mutant alters a corner that a cell with at least one
   new in-image pixel reads.
"""
import functools

import numpy as np

from oracle import hgi_numpy as N

LEFTTOP, CROSSED = N.LEFTTOP, N.CROSSED
TW = 128
TILE_HEIGHTS = (16, 32, 64)
OOB_MUTANTS = ("right", "below", "corner", "last_col", "last_row")
MUTANT_FILL = 0xC3


# ------------------------------------------------------------------------------------------------------ shape sets
def _r1():
    """One interior 128 x 64 tile followed by ragged tiles: (128 + c, 64 + r).  (column cross, row cross)"""
    cols = [(128 + c, 64 + r) for r in (64, 1, 38, 63) for c in range(1, 129)]
    rows = [(128 + c, 64 + r) for c in (128, 1, 67, 127) for r in range(1, 65)]
    return cols, rows


def _r0():
    """Frames smaller than a tile: (c, r)."""
    cols = [(c, r) for r in (64, 37) for c in range(1, 129)]
    rows = [(c, r) for c in (128, 67) for r in range(1, 65)]
    return cols, rows


def _unique(shapes):
    return list(dict.fromkeys(shapes))


D_COLS = (1, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
D_ROWS = (1, 16, 17, 32, 33, 63, 64, 65, 128, 129, 200)


@functools.lru_cache(maxsize=None)
def shape_set(name):
    """name -> list of (W, H), without repeats.  R1, R0: the remainder sets; R1c / R1r / R0c / R0r: their column and row
    crosses; R: both remainder sets; Rc, Rr: the crosses of both; D: the deep set."""
    if name in ("R1", "R1c", "R1r"):
        c, r = _r1()
        return _unique({"R1": c + r, "R1c": c, "R1r": r}[name])
    if name in ("R0", "R0c", "R0r"):
        c, r = _r0()
        return _unique({"R0": c + r, "R0c": c, "R0r": r}[name])
    if name == "R":
        return _unique(shape_set("R1") + shape_set("R0"))
    if name == "Rc":
        return _unique(shape_set("R1c") + shape_set("R0c"))
    if name == "Rr":
        return _unique(shape_set("R1r") + shape_set("R0r"))
    if name == "D":
        return [(128 + c, 64 + r) for c in D_COLS for r in D_ROWS]
    raise KeyError(name)


def content(w, h, batch=None, salt=0):
    """Seeded noise in [8, 255]: (h, w), or (batch, h, w)."""
    rng = np.random.default_rng(0x48474940 + 100003 * w + 1009 * h + salt)
    return rng.integers(8, 256, (h, w) if batch is None else (batch, h, w), dtype=np.uint8)


def filler(n, seed):
    """n nonzero random bytes: what lies around and between the rows of an input."""
    return np.random.default_rng(0x48474941 + seed).integers(1, 256, n, dtype=np.uint8)


def walk_cases():
    """The cases of the tile-walk suite (tests/test_tilewalk_gpu.py): (w, h, batch), every one under 1 MB."""
    out = []
    for ex in (1, 2, 3):
        for dw in (0, 5):
            for fy in (1, 2, 3, 4, 7, 8, 9, 16, 17, 24):
                for dh in (0, 3):
                    for batch in (1, 2, 3, 8, 9):
                        out.append((128 * ex + dw, 16 * fy + dh, batch))
    return out


# --------------------------------------------------------------------------------------------------- tile classes
def tile_classes(w, h, th):
    """The ragged tiles of a w x h frame under 128 x th tiles: one dict per tile whose body crosses the frame's edge.
    `edge`: the form of the check-free edge procedure the kernels pick for it (1: full width inside and even height)."""
    out = []
    fx, fy = w // TW, h // th
    for ty in range(-(-h // th)):
        for tx in range(-(-w // TW)):
            cols, rows = min(TW, w - tx * TW), min(th, h - ty * th)
            if cols == TW and rows == th:
                continue
            out.append(dict(cols=cols, rows=rows, cmod=cols % 16, even=h % 2 == 0, left=tx > 0 and ty < fy, above=ty > 0 and tx < fx,
                            edge=1 if cols == TW and h % 2 == 0 else 2))
    return out


# ----------------------------------------------------------------------------- the out-of-image rule, restated
def _lattice(img, step, mutant, fill=MUTANT_FILL):
    """oracle/hgi_numpy.py:_corner_lattice with the coordinates of every corner at hand: (values, altered).  `fill`: what the
    mutants `right`, `below` and `corner` read outside the image."""
    h, w = img.shape
    ny, nx = -(-h // step) + 1, -(-w // step) + 1
    cy, cx = np.arange(ny)[:, None] * step, np.arange(nx)[None, :] * step
    inside = (cy < h) & (cx < w)
    lat = np.zeros((ny, nx), np.int64)
    sub = img[::step, ::step]
    lat[: sub.shape[0], : sub.shape[1]] = sub
    if mutant is None:
        return lat, None
    if mutant == "right":
        hit, val = (cx >= w) & (cy >= 0), fill
    elif mutant == "below":
        hit, val = (cy >= h) & (cx >= 0), fill
    elif mutant == "corner":
        hit, val = (cx >= w) & (cy >= h), fill
    elif mutant == "last_col":
        hit, val = (cx == w - 1) & inside, 0
    elif mutant == "last_row":
        hit, val = (cy == h - 1) & inside, 0
    else:
        raise KeyError(mutant)
    lat[hit] = val
    return lat, hit


def _prediction(img, step, interp, mutant, fill=MUTANT_FILL):
    lat, _ = _lattice(img, step, mutant, fill)
    lt, rt, lb, rb = lat[:-1, :-1], lat[1:, :-1], lat[:-1, 1:], lat[1:, 1:]
    if interp == LEFTTOP:
        return lt.astype(np.uint8)
    avg = lambda a, b: (a + b + 1) >> 1
    return ((avg(lt, lb) + avg(rb, rt) + avg(rt, lt) + avg(rb, lb)) >> 2).astype(np.uint8)


def encode_oob(img, levels, lut, interp=CROSSED, mutant=None, fill=MUTANT_FILL):
    """oracle/hgi_numpy.py:encode on the lattice above."""
    img = np.ascontiguousarray(img, np.uint8)
    lut = np.asarray(lut, np.uint8)
    rec, grid = img.copy(), np.zeros_like(img)
    b = 1 << levels
    grid[::b, ::b] = img[::b, ::b]
    for level in range(levels):
        step = 1 << (levels - level)
        sub = step >> 1
        pred = _prediction(rec, step, interp, mutant, fill)
        for rv, gv in zip(N._level_views(rec, sub), N._level_views(grid, sub)):
            p = pred[: rv.shape[0], : rv.shape[1]]
            a = rv.copy()
            d = a - p
            q = lut[d]
            fb = ((p.astype(np.int64) + q) > 255) != (a < p)
            q = np.where(fb, d, q)
            gv[...] = q
            rv[...] = p + q
    return grid


def decode_oob(grid, levels, interp=CROSSED, mutant=None):
    """oracle/hgi_numpy.py:decode on the lattice above."""
    grid = np.ascontiguousarray(grid, np.uint8)
    out = np.zeros_like(grid)
    b = 1 << levels
    out[::b, ::b] = grid[::b, ::b]
    for level in range(levels):
        step = 1 << (levels - level)
        sub = step >> 1
        pred = _prediction(out, step, interp, mutant)
        for ov, gv in zip(N._level_views(out, sub), N._level_views(grid, sub)):
            ov[...] = pred[: ov.shape[0], : ov.shape[1]] + gv
    return out


def applies(mutant, w, h, levels):
    """Exact: at some level the mutant alters a corner of a cell that holds at least one new in-image pixel.  The cell at
    (x0, y0) of step s has the corners (x0, y0), (x0 + s, y0), (x0, y0 + s), (x0 + s, y0 + s) and the new pixels
    (x0 + s/2, y0), (x0, y0 + s/2), (x0 + s/2, y0 + s/2); x0 < w and y0 < h, so it holds a new in-image pixel exactly when
    x0 + s/2 < w or y0 + s/2 < h.  (The lattice holding an altered point is NOT enough: on a frame one pixel wide the cells
    of the last column have no new pixel to the right, and below the last row there is none either.)"""
    probe = np.zeros((h, w), np.uint8)
    for level in range(levels):
        step = 1 << (levels - level)
        sub = step >> 1
        _, hit = _lattice(probe, step, mutant)
        cell_hit = hit[:-1, :-1] | hit[1:, :-1] | hit[:-1, 1:] | hit[1:, 1:]
        y0, x0 = np.arange(cell_hit.shape[0])[:, None] * step, np.arange(cell_hit.shape[1])[None, :] * step
        live = (x0 + sub < w) | (y0 + sub < h)
        if bool((cell_hit & live).any()):
            return True
    return False
