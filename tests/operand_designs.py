"""Operand-coverage designs (a helper module of tests/test_operand_coverage*.py, not a conftest).

Three things, all defined from the reference restatement oracle/hgi_numpy.py and never from the library:

1. `encode_cov` / `decode_cov`: the whole-level algebra of oracle/hgi_numpy.py with recording added -- which (prediction,
   pixel) pairs every *site* of the per-pixel code sees and which corner quadruples the predictor of every level sees -- and
   with the six mutants of the quantizer step / the predictor that the designs must tell from the real rule.
2. Quantizer designs: frames of constant blocks whose new pixels of ONE level enumerate the pixel value, so that the level's
   prediction is the block's constant and every (p, a) pair reaches every site.
3. Predictor designs: images whose step lattices hold isolated cells with every corner quadruple over a set of edge values.

Sites: for sub = 1 and 2 a site is (sub, pixel family, x mod 16) -- the byte lane the pixel has in a 16-pixel chunk; for
sub >= 4 it is (sub, family).  Families: 0 right (x0 + sub, y0), 1 below (x0, y0 + sub), 2 diagonal (x0 + sub, y0 + sub).
"""
import functools

import numpy as np

from oracle import hgi_numpy as N

LEFTTOP, CROSSED = N.LEFTTOP, N.CROSSED
FAMILIES = ("right", "below", "diag")
V8 = (0, 1, 2, 127, 128, 253, 254, 255)            # corner values of the predictor designs at sub 1, 2, 4
V3 = (0, 128, 255)                                 # ... at deeper levels
S26 = tuple(sorted({0, 1, 2, 3, 126, 127, 128, 129, 252, 253, 254, 255} | set(range(0, 256, 16))))     # sub 8, 16
S8 = (0, 1, 127, 128, 254, 255, 64, 192)           # the levels above the tile (the cone)
ALL = tuple(range(256))
MUTANTS = ("ovf_ge", "borrow_le", "select_q_at_255", "avg_no_round", "sum_8bit", "lane_neighbour")


# ---------------------------------------------------------------------------------------------------------- tables
def tables():
    """name -> table; every one has lut[0] == 0 (a constant block reconstructs to itself, so p = c in the designs)."""
    ident = np.arange(256, dtype=np.uint8)
    one = ident.copy()
    one[255] = 254                                 # the LAST entry: an identity test that stops one short misses it
    rnd = np.random.default_rng(0x48474931).integers(0, 256, 256, dtype=np.uint8)
    rnd[0] = 0
    return {"linear1": N.linear_lut(1)[0], "linear2": N.linear_lut(2)[0], "linear3": N.linear_lut(3)[0], "identity": ident,
            "identity_but_255": one, "random0": rnd}


def table_nonzero_origin():
    """A random table with lut[0] != 0.  Outside the coverage condition (blocks do not stay constant under it); it exists because
    the borrow test `a < p` and its mutant `a <= p` differ at a == p only, where d = 0 and q = lut[0]: with lut[0] == 0 both
    q and the fallback d are 0 and the two rules are THE SAME FUNCTION.  Only a table with lut[0] != 0 can tell them apart."""
    t = np.random.default_rng(0x48474932).integers(0, 256, 256, dtype=np.uint8)
    t[0] = 37
    return t


# ------------------------------------------------------------------------------------- instrumented restatement
def site_keys(sub):
    step = 2 * sub
    if sub > 2:
        return [(sub, f) for f in range(3)]
    return [(sub, f, x) for f in range(3) for x in range(sub if f != 1 else 0, 16, step)]


class Coverage:
    """pairs[site]: 256 x 256 bool, [p, a] (decoder: [p, g]).  quads[sub]: bool over the quadruple classes of the level --
    index ((i_lt * n + i_rt) * n + i_lb) * n + i_rb with i_* the position in V8 (sub <= 4) or V3; a quadruple with a corner
    outside the set has no class.  Only cells whose three new pixels all lie in the frame are counted."""

    def __init__(self):
        self.pairs, self.quads = {}, {}

    def see_pairs(self, sub, fam, p, a):
        step = 2 * sub
        idx = p.astype(np.intp) * 256 + a
        if sub > 2:
            groups = [((sub, fam), idx)]
        else:
            ncls = 16 // step
            x_first = sub if fam != 1 else 0
            groups = [((sub, fam, (x_first + r * step) % 16), idx[:, r::ncls]) for r in range(ncls)]
        for key, ix in groups:
            tab = self.pairs.setdefault(key, np.zeros(65536, bool))
            tab[ix.reshape(-1)] = True

    def see_quads(self, sub, corners, nrow, ncol):
        vals = V8 if sub <= 4 else V3
        n = len(vals)
        code = np.full(256, -1, np.int64)
        code[list(vals)] = np.arange(n)
        cs = [code[c[:nrow, :ncol]] for c in corners]
        ok = (cs[0] >= 0) & (cs[1] >= 0) & (cs[2] >= 0) & (cs[3] >= 0)
        q = ((cs[0] * n + cs[1]) * n + cs[2]) * n + cs[3]
        tab = self.quads.setdefault(sub, np.zeros(n ** 4, bool))
        tab[q[ok]] = True

    def share(self, key):
        return float(self.pairs[key].mean()) if key in self.pairs else 0.0


def _prediction(img, step, interp, mutant):
    """oracle/hgi_numpy.py:_cell_prediction, returning the corners too; mutants `avg_no_round`, `sum_8bit`."""
    lat = N._corner_lattice(img, step)
    lt, rt, lb, rb = lat[:-1, :-1], lat[1:, :-1], lat[:-1, 1:], lat[1:, 1:]
    if interp == LEFTTOP:
        return lt.astype(np.uint8), (lt, rt, lb, rb)
    avg = lambda a, b: (a + b + 1) >> 1
    left = (lt + lb) >> 1 if mutant == "avg_no_round" else avg(lt, lb)
    right, top, bot = avg(rb, rt), avg(rt, lt), avg(rb, lb)
    total = left + right + top + bot
    if mutant == "sum_8bit":
        total = total & 255
    return (total >> 2).astype(np.uint8), (lt, rt, lb, rb)


def _family_prediction(pred, fam, sub, shape, mutant):
    p = pred[: shape[0], : shape[1]]
    if mutant == "lane_neighbour" and sub == 1 and fam == 0:       # x mod 16 == 5: cell column 2 of every eight
        other = np.concatenate([pred[:, 1:], pred[:, -1:]], axis=1)[: shape[0], : shape[1]]
        p = p.copy()
        lane = p[:, 2::8]
        lane[...] = np.where((lane == 0) | (lane == 255), other[:, 2::8], lane)
    return p


def encode_cov(img, levels, lut, interp=CROSSED, mutant=None, record=True):
    """oracle/hgi_numpy.py:encode with recording.  Returns (grid, reconstruction, Coverage).  `record`: True, False or the set
    of `sub` to record."""
    img = np.ascontiguousarray(img, np.uint8)
    lut = np.asarray(lut, np.uint8)
    rec, grid, cov = img.copy(), np.zeros_like(img), Coverage()
    if img.size == 0:
        return grid, rec, cov
    b = 1 << levels
    grid[::b, ::b] = img[::b, ::b]
    for level in range(levels):
        step = 1 << (levels - level)
        sub = step >> 1
        want = record is True or (record is not False and sub in record)
        pred, corners = _prediction(rec, step, interp, mutant)
        views = list(zip(N._level_views(rec, sub), N._level_views(grid, sub)))
        if want:
            cov.see_quads(sub, corners, *views[2][0].shape)
        for fam, (rv, gv) in enumerate(views):
            p = _family_prediction(pred, fam, sub, rv.shape, mutant)
            a = rv.copy()
            if want:
                cov.see_pairs(sub, fam, p, a)
            d = a - p
            q = lut[d]
            ovf = (p.astype(np.int64) + q) >= 255 if mutant == "ovf_ge" else (p.astype(np.int64) + q) > 255      # q > ~p
            exp = a <= p if mutant == "borrow_le" else a < p                  # (p + d > 255) <=> a < p
            fb = ovf != exp
            if mutant == "select_q_at_255":
                fb = fb & (p != 255)
            q = np.where(fb, d, q)
            gv[...] = q
            rv[...] = p + q
    return grid, rec, cov


def decode_cov(grid, levels, interp=CROSSED, mutant=None, record=True):
    """oracle/hgi_numpy.py:decode with recording: pairs are (p, g).  Returns (image, Coverage)."""
    grid = np.ascontiguousarray(grid, np.uint8)
    out, cov = np.zeros_like(grid), Coverage()
    if grid.size == 0:
        return out, cov
    b = 1 << levels
    out[::b, ::b] = grid[::b, ::b]
    for level in range(levels):
        step = 1 << (levels - level)
        sub = step >> 1
        want = record is True or (record is not False and sub in record)
        pred, corners = _prediction(out, step, interp, mutant)
        views = list(zip(N._level_views(out, sub), N._level_views(grid, sub)))
        if want:
            cov.see_quads(sub, corners, *views[2][0].shape)
        for fam, (ov, gv) in enumerate(views):
            p = _family_prediction(pred, fam, sub, ov.shape, mutant)
            if want:
                cov.see_pairs(sub, fam, p, gv)
            ov[...] = p + gv
    return out, cov


# ------------------------------------------------------------------------------------------- quantizer designs
def _round_up(v, m):
    return -(-v // m) * m


def block_geometry(sub, levels, n_values):
    """(block width, block height, cells per row, cell rows, x-classes) of one constant block that lets every x-class of level
    `sub` meet `n_values` pixel values.  Blocks start on multiples of B = max(2^levels, 16) and are multiples of B in size.

    The margin.  With b = 2^levels, the cells of the coarsest level in the block's last b columns (rows) have corners in the
    next block, so what they reconstruct is not c under a lossy table: after the level of step b the block's rows from bh - b on
    are polluted.  A cell predicts ALL its new pixels from all four corners, the one on its own top row too, so every finer level
    of step s carries the pollution one cell further up: after it the rows from bh - 2b + s on are polluted.  The targeted level
    (step 2 * sub) predicts from the state after step 4 * sub, so its corner rows must lie at or in front of bh - 2b + 2 * sub:
    a margin of almost two coarsest cells for the fine levels, of one for the coarsest level.  The smallest area wins."""
    step, b = 2 * sub, 1 << levels
    B = max(b, 16)
    ncls = max(1, 16 // step) if sub <= 2 else 1
    best = None
    for kw in range(2, 40):
        bw = kw * B
        ncx = (bw - 2 * b + step) // step // ncls * ncls
        if ncx <= 0:
            continue
        ncy = -(-n_values // (ncx // ncls))
        bh = _round_up(max((ncy - 1) * step + 2 * b, B), B)
        ncy = (bh - 2 * b + step) // step
        if best is None or bw * bh < best[0] * best[1]:
            best = (bw, bh, ncx, ncy, ncls)
    return best


def _block(sub, levels, c, avals):
    bw, bh, ncx, ncy, ncls = block_geometry(sub, levels, len(avals))
    step = 2 * sub
    blk = np.full((bh, bw), c, np.uint8)
    j, i = np.arange(ncy)[:, None], np.arange(ncx)[None, :]
    a = np.asarray(avals, np.uint8)[(j * (ncx // ncls) + i // ncls) % len(avals)]       # by cell row, shifted by cell column
    blk[0:ncy * step:step, sub:ncx * step:step] = a
    blk[sub:ncy * step:step, 0:ncx * step:step] = a
    blk[sub:ncy * step:step, sub:ncx * step:step] = a
    return blk


def quantizer_frame(levels, targets):
    """One frame for a pyramid of `levels`: for every (sub, c values, a values) of `targets` a group of constant blocks, 16 per
    row at most, the groups below one another.  Unused area is 0."""
    groups = []
    for sub, cvals, avals in targets:
        blocks = [_block(sub, levels, c, avals) for c in cvals]
        per_row = min(16, len(blocks))
        rows = [np.concatenate(blocks[k:k + per_row], axis=1) for k in range(0, len(blocks), per_row)]
        width = max(r.shape[1] for r in rows)
        rows = [np.pad(r, ((0, 0), (0, width - r.shape[1]))) for r in rows]
        groups.append(np.concatenate(rows, axis=0))
    width = max(g.shape[1] for g in groups)
    return np.ascontiguousarray(np.concatenate([np.pad(g, ((0, 0), (0, width - g.shape[1]))) for g in groups], axis=0))


# name -> (frame levels, targets, [levels the frame is run at]).  A frame built for 2^5 margins serves every shallower pyramid:
# its blocks start on multiples of 32 and its margins are at least one coarsest cell of any of them.
QUANT_FRAMES = {
    "q1": (5, ((1, ALL, ALL),), (1, 2, 3, 4, 5)),
    "q2": (5, ((2, ALL, ALL),), (2, 3, 4, 5)),
    "q4": (5, ((4, ALL, ALL),), (3, 4, 5)),
    "q8_16": (5, ((8, S26, S26), (16, S26, S26)), (5,)),
    "cone6": (6, ((16, S8, S8), (32, S8, S8)), (6,)),
    "cone7": (7, ((16, S8, S8), (32, S8, S8), (64, S8, S8)), (7,)),
    "cone8": (8, ((16, S8, S8), (32, S8, S8), (64, S8, S8), (128, S8, S8)), (8,)),
}


@functools.lru_cache(maxsize=None)
def quant_frame(name):
    levels, targets, _ = QUANT_FRAMES[name]
    f = quantizer_frame(levels, targets)
    f.setflags(write=False)
    return f


def quant_designs():
    """[(design name, frame name, levels, ((sub, values), ...))]: the (sub, value set) pairs whose product must be covered."""
    out = []
    for name, (_, targets, runs) in QUANT_FRAMES.items():
        for lv in runs:
            req = tuple((sub, avals) for sub, _, avals in targets if sub < (1 << lv))
            out.append(("%s_L%d" % (name, lv), name, lv, req))
    return out


def required_pairs(values):
    """The 256 x 256 bool mask of values x values, flattened like Coverage.pairs."""
    m = np.zeros(256, bool)
    m[list(values)] = True
    return (m[:, None] & m[None, :]).reshape(-1)


# ------------------------------------------------------------------------------------------- predictor designs
# A 10 x 11 lattice over the positions of V3 whose ninety 2 x 2 windows hold all 81 quadruples (found by a seeded hill climb;
# test_operand_coverage.py asserts the property).
WINDOW_LATTICE = ("00021202022", "01201111120", "22201102022", "22100110100", "01021221022", "02002111012", "22102212212",
                  "10010201120", "00012120000", "11112102002")


def _isolated_region(sub):
    """All 4096 quadruples over V8 on isolated cells of step 2 * sub (every other cell column and row), once for every x-class
    of the cell: copy (s, r) puts quadruple n into slot column n % 64 + r of slot row n // 64, the slots' cells at column
    2 * slot + s.  Returns one (values, mask) per copy: only lattice points are set."""
    step = 2 * sub
    ncls = max(1, 16 // step) if sub <= 2 else 1
    copies = [(s, r) for s in range(2) for r in range(ncls // 2)] if ncls > 1 else [(0, 0)]
    v = np.asarray(V8, np.uint8)
    n = np.arange(4096)
    q = [v[(n >> 9) & 7], v[(n >> 6) & 7], v[(n >> 3) & 7], v[n & 7]]          # lt, rt, lb, rb
    ch = 2 * 64 * step + 1
    cw = _round_up((2 * (63 + max(1, ncls // 2)) + 2) * step + 1, 16)
    out = []
    for s, r in copies:
        val, mask = np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), bool)
        x0 = (2 * (n % 64 + r) + s) * step
        y0 = 2 * (n // 64) * step
        for (dy, dx), c in zip(((0, 0), (step, 0), (0, step), (step, step)), q):       # rt is (x0, y0 + step), lb (x0 + step, y0)
            val[y0 + dy, x0 + dx] = c
            mask[y0 + dy, x0 + dx] = True
        out.append((val, mask))
    return out


def _lattice_region(sub):
    """All 81 quadruples over V3 on step 2 * sub: WINDOW_LATTICE laid on the step lattice, 9 x 10 cells."""
    step = 2 * sub
    lat = np.asarray(V3, np.uint8)[np.array([[int(ch) for ch in row] for row in WINDOW_LATTICE])]
    rows, cols = lat.shape
    val = np.zeros(((rows - 1) * step + 1, (cols - 1) * step + 1), np.uint8)
    mask = np.zeros(val.shape, bool)
    val[::step, ::step] = lat
    mask[::step, ::step] = True
    return [(val, mask)]


def predictor_image(levels, width):
    """The decoded image D of a predictor design: seeded noise with the regions of every level packed on shelves (tallest first),
    each region on a multiple of its own step and of 16.  Every image ends on an odd width and height."""
    regions = []
    for k in range(levels):
        sub = 1 << k
        regions += [(max(16, 2 * sub),) + r for r in (_isolated_region(sub) if sub <= 4 else _lattice_region(sub))]
    regions.sort(key=lambda r: -r[2].shape[0])
    placed, x, y, shelf = [], 0, 0, 0
    for align, val, mask in regions:
        h, w = mask.shape
        assert w <= width
        x = _round_up(x, align)
        if x + w > width:
            x, y, shelf = 0, y + shelf, 0
        top = _round_up(y, align)
        placed.append((top, x, val, mask))
        shelf = max(shelf, top + h - y)
        x += w
    d = np.random.default_rng(0x48474933 + levels).integers(0, 256, ((y + shelf) | 1, width | 1), dtype=np.uint8)
    for top, x, val, mask in placed:
        h, w = mask.shape
        d[top:top + h, x:x + w][mask] = val[mask]
    return d


PRED_FRAMES = {"pred5": (5, 2112), "pred8": (8, 4224)}


@functools.lru_cache(maxsize=None)
def pred_frame(name):
    f = predictor_image(*PRED_FRAMES[name])
    f.setflags(write=False)
    return f


def required_quads(sub):
    return len(V8 if sub <= 4 else V3) ** 4


# -------------------------------------------------------------------------------------------------- noise cases
def noise_case(levels=8):
    """The largest noise case of tests/test_parity_gpu.py::test_random_shapes_and_tables in its class, with its seed."""
    w, h = 1280, 640
    return np.random.default_rng(w * 7919 + h * 31 + 8).integers(0, 256, (h, w), dtype=np.uint8), levels
