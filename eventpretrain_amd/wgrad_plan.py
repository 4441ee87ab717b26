"""Launch planner of the deferred weight / bias gradients: which grouped entry each queued problem goes to, in which launch
and round, cut into which K-slices, and the tables of those launches with every field but the addresses. Integers and numpy
only: the queued operands are opaque here, ops._DeferredGrads binds them (allocates, fills the pointer fields, stages).

Table formats as in include/evtpretrain.h:186-205 (problems, 64 bytes) and :246-250 (column sums, 40 bytes); an item is
4 x int32 (prob, tile_m | col_block, tile_n | row_slab, pad). They are stated here and nowhere else in Python."""
from typing import Any, NamedTuple

import numpy as np

PROBLEM_DT = np.dtype([("A", "<u8"), ("B", "<u8"), ("C", "<u8"), ("M", "<i4"), ("N", "<i4"), ("K", "<i4"), ("lda", "<i4"),
                       ("ldb", "<i4"), ("ldc", "<i4"), ("acc", "<i4"), ("cacc", "<i4"), ("colsum", "<u8")])
COLSUM_DT = np.dtype([("x", "<u8"), ("out", "<u8"), ("M", "<i8"), ("N", "<i4"), ("ld", "<i4"), ("dtype", "<i4"), ("pad", "<i4")])
G4 = "evp_gemm_grouped_tn_g4_bf16"          # 256x256 output tiles
T128 = "evp_gemm_grouped_tn_bf16"           # 128x128 output tiles
COLSUM = "evp_colsum_grouped"               # blocks of 128 columns x 256 rows
ENTRY = {256: G4, 128: T128}
COLSUM_COLS, COLSUM_ROWS = 128, 256

G4_CONTRACT = "K % 32 == 0, K >= 96, M, N >= 256, N % 8 == 0"


def g4_ok(M, N, K):
    """The G4 grouped body's contract (include/evtpretrain.h): its prologue consumes three 32-row stages with unbounded buffer
    resources whatever K is, and its tables live on the device, where nothing checks them."""
    return K % 32 == 0 and K >= 96 and M >= 256 and N >= 256 and N % 8 == 0


class WgradProblem(NamedTuple):
    """One queued dW[n_out, k_in] = dy^T x over `rows` rows; `bias`: the same Linear's bias, whose gradient sum_rows(dy) rides
    along. The planner reads the three integers, id(param) and whether there is a bias; the rest is the binder's."""
    param: Any
    dy: Any
    x: Any
    n_out: int
    k_in: int
    rows: int
    bias: Any = None


class Route(NamedTuple):
    """Where one problem goes, decided once by route() and carried with the problem."""
    tile: int           # 256: the G4 entry, 128: the 128x128 entry
    slices: tuple       # ((k0, k), ...) partition of the rows; more than one: each slice writes a workspace, summed afterwards
    bias: str           # "fused" into the G4 problem | "listed" in the grouped column sums | "none"


def route(n_out, k_in, rows, has_bias, use_g4):
    # long-K problems with >= 256-wide outputs go to the 256x256 G4 kernel
    tile = 256 if use_g4 and g4_ok(n_out, k_in, rows) else 128
    tiles = ((n_out + tile - 1) // tile) * ((k_in + tile - 1) // tile)
    slices = ((0, rows),)
    # A problem with few output tiles and a very long K (ConvViT stage 1: 256x256 outputs, K = B*56*56) would keep one
    # workgroup busy for the whole launch: cut its K into slices that run as separate problems into a workspace and are
    # summed afterwards.
    if tiles <= 32 and rows >= 32768 and (n_out * k_in) % 4 == 0:
        ns = min(64, rows // 8192)
        kper = ((rows // 64 + ns - 1) // ns) * 64
        ns = (rows + kper - 1) // kper
        if tile == 256 and not g4_ok(n_out, k_in, rows - (ns - 1) * kper):
            ns -= 1                 # a G4 slice needs K >= 96: the short tail joins the slice before it
        slices = tuple((s * kper, rows - s * kper if s == ns - 1 else kper) for s in range(ns))
    # a bias gradient rides on its Linear's weight-gradient problem only in the 256x256 kernel and only unsliced; otherwise
    # it joins the grouped column sums
    bias = "none" if not has_bias else "fused" if tile == 256 and len(slices) == 1 else "listed"
    return Route(tile, slices, bias)


class Member(NamedTuple):
    """A queued problem with its routing."""
    q: WgradProblem
    route: Route


class Row(NamedTuple):
    """One row of a problem table with symbolic operands: rows [k0, k0 + k) of members[src]'s dy and x, written to slice
    `ws_slice` of that member's split-K workspace, or to its gradient (ws_slice < 0)."""
    src: int
    k0: int
    k: int
    ws_slice: int


class Launch(NamedTuple):
    tag: str            # staging key, unique within a plan
    entry: str
    round: int          # launches of one round write disjoint gradients (may run concurrently); rounds are ordered
    members: list       # the queued problems of this launch, longest K first
    rows: list          # Row per table row, longest K first
    probs: np.ndarray   # PROBLEM_DT, one per row: sizes and leading dimensions set, addresses and accumulate flags zero
    items: np.ndarray   # int32 [n_items, 4]


def _grid(prob, n_outer, n_inner):
    """[n_outer, n_inner, 4] items (prob, inner index, outer index, 0)"""
    t = np.zeros((n_outer, n_inner, 4), dtype=np.int32)
    t[..., 0] = prob
    t[..., 1] = np.arange(n_inner, dtype=np.int32)[None, :]
    t[..., 2] = np.arange(n_outer, dtype=np.int32)[:, None]
    return t


def _launch(tag, r, members, tile, xcd_order):
    rows = [Row(src, k0, k, s if len(rt.slices) > 1 else -1)
            for src, (_, rt) in enumerate(members) for s, (k0, k) in enumerate(rt.slices)]
    rows.sort(key=lambda row: -row.k)           # longest K first
    probs = np.zeros(len(rows), dtype=PROBLEM_DT)
    xcd_order = xcd_order and tile == 256
    items, weights = [], []
    for i, row in enumerate(rows):
        q = members[row.src].q
        probs[i] = (0, 0, 0, q.n_out, q.k_in, row.k, q.n_out, q.k_in, q.k_in, 0, 0, 0)
        tm, tn = (q.n_out + tile - 1) // tile, (q.k_in + tile - 1) // tile
        t = _grid(i, tn, tm)
        if xcd_order:
            t = _supertile_major(t, 2, 4)
        items.append(t.reshape(-1, 4))
        weights.append(np.full(tm * tn, float(row.k), dtype=np.float64))
    items = np.concatenate(items, 0)
    if xcd_order:
        items = _deal_to_xcds(items, np.concatenate(weights))
    return Launch(tag, ENTRY[tile], r, members, rows, probs, items)


def layout(w, n_chunks, use_g4, xcd_order):
    """w: the queued WgradProblems -> (launches, listed): the GEMM launches in order, and the problems whose bias gradient
    goes to the grouped column sums, in the order they join that list."""
    routed = [Member(q, route(q.n_out, q.k_in, q.rows, q.bias is not None, use_g4)) for q in w]
    listed = [m.q for m in routed if m.route.bias == "listed" and m.route.tile == 128]
    # A parameter used by several autograd nodes of one backward (rec+con: masked AND dense forward) has several queued
    # contributions. Tiles of different problems run concurrently, so contributions to the SAME gradient go to successive
    # launches (round r holds every parameter's r-th contribution; normally one round).
    rounds, count = [], {}
    for m in routed:
        r = count.get(id(m.q.param), 0)
        count[id(m.q.param)] = r + 1
        while len(rounds) <= r:
            rounds.append([])
        rounds[r].append(m)
    launches = []
    for r, batch in enumerate(rounds):
        # per round: the 256x256 ring kernel (in n_chunks launches when a plan is built) and the 128x128 kernel; inside a
        # launch the longest-K tiles are listed first
        big = sorted([m for m in batch if m.route.tile == 256], key=lambda m: -m.q.rows)
        small = sorted([m for m in batch if m.route.tile == 128], key=lambda m: -m.q.rows)
        if big:
            k = max(1, min(n_chunks if r == 0 else 1, len(big)))
            work = np.cumsum([float(m.q.n_out) * m.q.k_in * m.q.rows for m in big])
            cuts = [0] + [int(np.searchsorted(work, work[-1] * (c + 1) / k, side="left")) + 1 for c in range(k - 1)] + [len(big)]
            cuts = sorted(set(min(max(c, 0), len(big)) for c in cuts))
            for c in range(len(cuts) - 1):
                part = big[cuts[c]:cuts[c + 1]]
                listed += [m.q for m in part if m.route.bias == "listed"]
                launches.append(_launch("w256r%dc%d" % (r, c), r, part, 256, xcd_order))
        if small:
            launches.append(_launch("w128r%d" % r, r, small, 128, xcd_order))
    return launches, listed


def colsum_items(shapes):
    """Items of the grouped column sums over tensors of the given (M, N) shapes."""
    return np.concatenate([_grid(i, (M + COLSUM_ROWS - 1) // COLSUM_ROWS, (N + COLSUM_COLS - 1) // COLSUM_COLS).reshape(-1, 4)
                           for i, (M, N) in enumerate(shapes)], 0)


def _supertile_major(t, sm, sn):
    """[tn, tm, 4] tile grid -> the same tiles listed super-tile by super-tile (sn x sm tiles each, tile_m fastest inside):
    the 8 tiles of a 2 x 4 super-tile read 2 A panels and 4 B panels between them instead of 16."""
    tn, tm = t.shape[0], t.shape[1]
    out = []
    for n0 in range(0, tn, sn):
        for m0 in range(0, tm, sm):
            out.append(t[n0:n0 + sn, m0:m0 + sm].reshape(-1, 4))
    return np.concatenate(out, 0)


def _deal_to_xcds(items, work, n_xcd=8):
    """Workgroups b and b + 8 run on the same XCD (one L2 each; MI355X_MICROARCH.md, workgroup dispatch) and an XCD's CUs
    take its workgroups in launch order. Cut the item sequence (super-tile major, longest K first) into 8 CONTIGUOUS runs of
    equal estimated work (tiles x K) and interleave them, items[8 k + x] = run_x[k], so that the ~32 tiles an XCD runs at any
    moment are neighbouring super-tiles of one problem -- they advance through K in lockstep and find each other's panels in
    their L2 instead of re-reading them through the Infinity Cache (2.9x over-fetch measured in round 1). Short runs are
    padded with prob = -1 items, which the kernels skip. Placement is speed only: any assignment gives the same result."""
    n = items.shape[0]
    if n < 4 * n_xcd:
        return items
    cum = np.cumsum(work)
    cuts = [0] + [int(np.searchsorted(cum, cum[-1] * (x + 1) / n_xcd, side="left")) + 1 for x in range(n_xcd - 1)] + [n]
    cuts = [min(max(c, 0), n) for c in cuts]
    for i in range(1, len(cuts)):
        cuts[i] = max(cuts[i], cuts[i - 1])
    runs = [items[cuts[x]:cuts[x + 1]] for x in range(n_xcd)]
    longest = max(r.shape[0] for r in runs)
    out = np.full((longest, n_xcd, 4), -1, dtype=np.int32)
    for x, r in enumerate(runs):
        out[:r.shape[0], x] = r
    return out.reshape(-1, 4)
