"""Inputs of test_wide_conformance.py: pattern forests that hold the thresholds of the wide-node kernel (k1w_kernel), of the second level
(l2_*) and of the sorts and stream jobs behind them on purpose, and a census on the host that proves it before anything runs on a device.

Everything is compared with the flat-form definition in numpy (variant_cases.definition), never with a second run of the engine.

The families are written in BLOCK UNITS: a cell (b, p) is the id at position p < 32 of logical block b < 36, and logical block b is the
block b * stride of the database — so the same families exist at any block width >= 32 (`width`) and spread over any number of blocks
(`stride`).  The generator adds the nodes in DFS pre-order (a node's whole subtree before its next sibling: pattern ids ascend along the
pre-order, which is the order the engine's layout gives them — children in pid order, roots ascending), so that it knows the position of
every node in the wide list while it builds and can pad to the batch and run boundaries it wants.  The census does not rely on that: it
computes the pre-order from the parent links."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import variant_cases as V  # noqa: E402

# the engine's constants that the families aim at (a2a_blocks.hip)
WAVE = 64
K1W_HEAVY = 11
K1W_OXCAP = 96
K1W_ARENA_MIN = 256
L2_MIN_DEFAULT = 24
L2_QCAP = 576
L2_NODE_GRAB, L2_SUB = 16, 16
CS_MAX_KEYS = 2048
CS_TILE = 2048
K2J_REC = 16384
CH_REC = 256
RS_JOB_CHUNKS = 64

LOGICAL_BLOCKS = 36                                   # 35 blocks of ids and a last one of which only position 0 is used
CS_FULL = (3, 4, 10, 11, 12, 23, 24, 25, 35)
CS_SMALL = (3, 11, 24)
SIB_FULL = (1, 63, 64, 65, 127, 128, 129)
SIB_SMALL = (1, 63, 64, 65)
JOIN_WEIGHTS = (1, 127, 128, 16383, 16384, 1 << 28, (1 << 32) - 1)
SOURCES = ("NONE", "FN1", "FN2", "LANE", "CHAIN_SAME_RUN", "CHAIN_EARLIER_RUN")


def arena_cap(NB):
    return max(K1W_ARENA_MIN, (NB + 2 + 63) // 64 * 64)


# ------------------------------------------------------------------------------------------------------------------------------------
# the builder: a _Forest in block units that knows the wide list as it grows
# ------------------------------------------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, width, stride=1, light=False):
        assert width >= 32 and stride >= 1
        self.F, self.width, self.stride, self.light = V._Forest(), width, stride, light
        self.blocks = [frozenset()]                   # logical blocks of every node's full list
        self.path = []                                # the root path of the node added last
        self.pos = 0                                  # wide nodes so far
        self.n = 0

    def wt(self, zero_ok=True):
        """the next weight: variant_cases.WEIGHTS in turn (light: 1 .. 127 in turn, every node acts)"""
        self.n += 1
        if self.light:
            return 1 + (self.n * 37) % 127
        w = V.WEIGHTS[self.n % len(V.WEIGHTS)]
        return w if w or zero_ok else 3

    def add(self, cells, parent, w):
        assert all(0 <= b < LOGICAL_BLOCKS and 0 <= p < 32 and (b < LOGICAL_BLOCKS - 1 or p == 0) for b, p in cells), cells
        while self.path and self.path[-1] != parent:
            self.path.pop()
        assert (parent < 0 and not self.path) or (self.path and self.path[-1] == parent), "nodes are added in DFS pre-order"
        if self.light:
            w = 1 + (7 * len(self.F.locs) + w % 5) % 127
        p = self.F.add([b * self.stride * self.width + q for b, q in cells], parent, w)
        self.path.append(p)
        blk = (self.blocks[parent] if parent >= 0 else frozenset()) | frozenset(b for b, _ in cells)
        self.blocks.append(blk)
        self.pos += len(blk) > 2
        return p

    def filler_root(self):
        """a root of three blocks, one id each"""
        i = self.n
        self.n += 1
        b = i % (LOGICAL_BLOCKS - 3)
        return self.add([(b, i % 32), (b + 1, (i // 3) % 32), (b + 2, (i // 7) % 32)], -1, 1 + i % 5)

    def pad_roots(self, rem, mod):
        while self.pos % mod != rem:
            self.filler_root()

    def filler_leaf(self, R, last_block, above):
        """a one-id child of the wide node R in R's last block (a seam, no new block), above R's own ids there"""
        i = self.n
        self.n += 1
        return self.add([(last_block, above + 1 + i % (31 - above))], R, 1 + i % 3)


def _target_shapes(pc, cs):
    """(own pairs, seam) of the children of a node of pc blocks whose block count pc + pairs - seam is one of cs"""
    return [(k, seam) for k in (1, 2, 5, 6) for seam in (0, 1) if pc + k - seam in cs]


def _add_target(B, R, pc, k, seam, acting=True):
    """a child of chain node R (blocks 0 .. pc - 1, its last id at position 1 of block pc - 1) with k own pairs: the first in R's last
    block (seam) or in a new one; every fourth further pair and every third seam pair with two ids (a diagonal record), the others with one"""
    j = B.n
    fb = pc - 1 if seam else pc
    cells = []
    for t in range(k):
        b = fb + t
        if seam and t == 0:
            cells += [(b, 4 + j % 20)] + ([(b, 30)] if j % 3 == 0 else [])
        elif b == LOGICAL_BLOCKS - 1:
            cells += [(b, 0)]
        else:
            cells += [(b, 2)] + ([(b, 9)] if (j + t) % 4 == 0 else [])
    return B.add(cells, R, B.wt(zero_ok=not acting))


def _family_edges(B):
    """wide nodes at positions 63, 64, 65 and 255, 256, 257 of the wide list, each the child of the one before: a wide parent at lane 63 with
    its child at lane 0 of the next batch (and of the next run of 64 / of 256), a grandchild at lane 1; between them a batch of 64 acting
    roots whose rows are exactly 256 entries"""
    for at in (63, 255):
        B.pad_roots(at % 256, 256)
        assert B.pos == at
        r = B.add([(3, 0), (4, 0), (4, 1), (5, 0)], -1, 128)
        c = B.add([(6, 1), (6, 2)], r, 127)
        B.add([(6, 5), (7, 0)], c, 65536)
        if at == 63:
            _family_arena(B, 4)


def _family_arena(B, blocks):
    """a batch of 64 acting wide nodes under narrow parents (odd lanes) or none (even lanes), `blocks` blocks each: rows of 64 * blocks entries"""
    B.pad_roots(0, 64)
    first = B.pos
    for i in range(64):
        s = (5 * i) % (LOGICAL_BLOCKS - 1 - blocks)
        if i % 2 == 0:
            B.add([(s + t, (i + t) % 32) for t in range(blocks)] + ([(s, 31)] if i % 4 == 0 else []), -1, B.wt(zero_ok=False))
        else:
            nar = B.add([(s, 0), (s, 1 + i % 8)], -1, B.wt())
            B.add([(s + t, 10 + (i + t) % 20) for t in range(1, blocks)], nar, B.wt(zero_ok=False))
    assert B.pos == first + 64


def _family_ox(B, over):
    """a batch of 64 wide nodes, 32 roots each with a child: exactly K1W_OXCAP further own pairs (roots of four own pairs, children of one),
    or 128 (three own pairs everywhere: the further pairs of the lanes from 48 on find no room, and the children among them walk through
    their parents' pairs in memory)"""
    B.pad_roots(0, 64)
    first = B.pos
    for i in range(32):
        s = (3 * i) % (LOGICAL_BLOCKS - 8)
        if over:
            r = B.add([(s, i % 32), (s + 1, 0), (s + 1, 1 + i % 9), (s + 2, 3)], -1, B.wt())
            B.add([(s + 2, 4 + i % 8), (s + 3, 0), (s + 4, i % 32)], r, B.wt(zero_ok=False))
        else:
            r = B.add([(s, i % 32), (s + 1, 0), (s + 2, 1 + i % 9), (s + 3, 3)], -1, B.wt())
            B.add([(s + 3, 4 + i % 8)] if i % 2 else [(s + 4, i % 32)], r, B.wt(zero_ok=False))
    assert B.pos == first + 64


def _chain_down(B, cs, lane_targets):
    """the chain R3 (a root over blocks 0, 1, 2), R4, ..., R35: R_pc has pc blocks and adds position 1 of block pc - 1.  With lane_targets,
    every R_pc is followed at once by its target children (they share its batch: wide parent in the batch), then by R_(pc+1)."""
    chain = []
    for pc in range(3, LOGICAL_BLOCKS):
        shapes = _target_shapes(pc, cs) if lane_targets else []
        if chain and B.pos % 64 + 1 + len(shapes) > 64:
            while B.pos % 64:
                B.filler_leaf(chain[-1][0], pc - 2, 1)
        R = B.add([(0, 0), (1, 0), (2, 1)] if pc == 3 else [(pc - 1, 1)], chain[-1][0] if chain else -1, B.wt())
        chain.append((R, pc))
        for k, seam in shapes:
            _add_target(B, R, pc, k, seam)
    return chain


def _chain_up(B, chain, cs):
    """the target children of every chain node again, deepest node first, after the deeper part of the chain: wide parent in an earlier batch"""
    for R, pc in reversed(chain):
        for k, seam in _target_shapes(pc, cs):
            _add_target(B, R, pc, k, seam)


def _family_sources(B, cs, far):
    """every block count of cs under a wide parent: in the parent's batch, in a later batch of the parent's run of 256, and (far) in a later
    run — each with every shape (own pairs 1, 2, 5 or 6; seam or not) that the block count allows"""
    B.pad_roots(0, 256)
    chain = _chain_down(B, cs, True)
    while B.pos % 64:
        B.filler_leaf(chain[-1][0], LOGICAL_BLOCKS - 2, 1)
    _chain_up(B, chain, cs)
    if far:
        B.pad_roots(128, 256)
        chain = _chain_down(B, cs, False)
        while B.pos % 256:
            B.filler_leaf(chain[-1][0], LOGICAL_BLOCKS - 2, 1)
        _chain_up(B, chain, cs)


def _family_narrow_parents(B, cs):
    """every block count of cs as a root, and under a parent of one block and of two blocks, with a seam and without; one of the parents has no weight"""
    for n, c in enumerate(cs):
        s = (7 * n) % (LOGICAL_BLOCKS - c + 1)
        top = s + c - 1
        cell = lambda b, p: (b, 0 if b == LOGICAL_BLOCKS - 1 else p)          # noqa: E731
        B.add(sorted(set([cell(b, n % 5) for b in range(s, top + 1)] + [cell(s + 1, 20)])), -1, B.wt(zero_ok=False))
        p1 = B.add([(s, 0), (s, 1)], -1, 0 if n % 2 else B.wt())
        B.add([cell(b, 2) for b in range(s + 1, top + 1)], p1, B.wt(zero_ok=False))
        B.add([(s, 5)] + [cell(b, 3 + (b % 2) * 4) for b in range(s + 1, top + 1)] + [cell(s + 1, 30)], p1, B.wt(zero_ok=False))
        p2 = B.add([(s, 3), (s + 1, 1)], -1, B.wt())
        B.add([cell(b, 2) for b in range(s + 2, top + 1)], p2, B.wt(zero_ok=False))
        B.add([(s + 1, 5), (s + 1, 6)] + [cell(b, 4) for b in range(s + 2, top + 1)], p2, B.wt(zero_ok=False))


def _family_shared_chain(B, length, sib_depths):
    """a root path of `length` wide one-id nodes below a one-block root, a node without weight and a two-block node; chain node i adds id 7 i
    of the blocks from 2 on (a new block or a seam, as it comes).  Children hang off the chain nodes of depth d in sib_depths (depth 1: the
    first wide node): one in front of the deeper chain (same batch), three after it (the chain list shared across batches and runs) of which
    one has a child of its own.  The first wide node sits at position 156 of a run of 256: the run boundaries of 64 and of 256 nodes fall on
    chain nodes with some 35 and some 100 wide ancestors — the scan at a run's start takes a second pass."""
    a1 = B.add([(0, 0), (0, 1)], -1, 3)
    a0 = B.add([(0, 2)], a1, 0)
    par = B.add([(1, 0)], a0, 5)
    chain = []
    cellof = lambda i: (2 + (7 * i) // 32, (7 * i) % 32)                  # noqa: E731
    for i in range(length):
        b, p = cellof(i)
        par = B.add([(b, p)], par, B.wt())
        chain.append(par)
        if i + 1 in sib_depths and p < 31:
            B.add([(b, p + 1)] if i % 2 else [(b + 1, 0), (b + 1, 5)], par, B.wt(zero_ok=False))
    for d in sorted(sib_depths, reverse=True):
        b, p = cellof(d - 1)
        R = chain[d - 1]
        if p < 31:
            B.add([(b, p + 1)], R, B.wt(zero_ok=False))                                        # seam
        x = B.add([(b + 1, 1), (b + 2, 0), (b + 2, 3)], R, B.wt(zero_ok=False))                     # two new blocks
        B.add([(b + 2, 9)], x, B.wt(zero_ok=False))
        B.add([(b, p + 1)] * (p < 31) + [(b + 1, 2), (b + 2, 1), (b + 3, 0), (b + 3, 1)], R, B.wt(zero_ok=False))


def _every_block_patterns(F, width, N):
    """two patterns with one id in every block of the database, the first with a chain of one-id children at the top end (ids ascend along a root
    path: a chain below such a root grows at the top end only)"""
    NB = (N + width - 1) // width
    size = lambda X: min(width, N - X * width)                  # noqa: E731
    short = size(NB - 1) < 8                                    # a last block that cannot hold the chain: the chained root leaves it to its last child
    r = F.add([X * width + 5 for X in range(NB - 1 if short else NB)], -1, 3)
    top = int(F.locs[r][-1])
    par = r
    for j in range(1, 8):
        par = F.add([top + j], par, (2, 0, 127, 128, 1, 255, 3)[j % 7])
    if short:
        F.add([N - 1], par, 129)
    F.add([X * width + (size(X) - 1) for X in range(NB)], -1, 128)


def wide_forest(N=35 * 32 + 1, width=32, size="full", light=False):
    """The wide families over ceil(N / width) blocks (36 of them for the default N at width 32; more: the 36 logical blocks are spread with a
    stride).  size "small": the block counts 3 / 11 / 24 and a chain of 70 only, plus two patterns with one id in EVERY block.  light: every
    weight in 1 .. 127 (one base-128 digit: a record per block pair)."""
    NB = (N + width - 1) // width
    assert NB >= LOGICAL_BLOCKS and N >= (LOGICAL_BLOCKS - 1) * width + 1
    full = size == "full"
    B = _Builder(width, (NB - 1) // (LOGICAL_BLOCKS - 1), light)
    cs = CS_FULL if full else CS_SMALL
    _family_edges(B)                                           # positions 63 .. 65, a batch of 256 row entries, positions 255 .. 257
    _family_arena(B, 5)                                        # 320 row entries: two rounds of the arena
    _family_ox(B, False)
    _family_ox(B, True)
    _family_sources(B, cs, far=full)
    _family_narrow_parents(B, cs)
    B.pad_roots(156, 256)
    _family_shared_chain(B, 135 if full else 70, SIB_FULL if full else SIB_SMALL)
    if not full:
        _every_block_patterns(B.F, width, N)
    return B.F.pat()


def join_forest(width=32):
    """40 blocks.  700 nodes of 11 blocks that all contain blocks 3 and 7 — roots, and every fifth a child of the one before it with one more id
    in its last block — so the tiles (7, 3), (3, 3) and (7, 7) get more than L2_QCAP matches and (with indices handed out densely) whole bitmap
    words of ones; 70 nodes of 11 blocks that share exactly ONE block pair with them, (3, 3) (they hold block 3 and ten of the blocks 24 .. 39,
    the 700 hold blocks below 24 only); the weights cycle through one, two, three and five base-128 digits, and the 700 nodes add up past 2^32
    in the cells of blocks 3 and 7."""
    F = V._Forest()
    others = [b for b in range(24) if b not in (3, 7)]
    prev = -1
    for i in range(700):
        w = JOIN_WEIGHTS[i % len(JOIN_WEIGHTS)]
        if i % 5 == 4 and prev >= 0:
            last = int(F.locs[prev][-1])
            if (last + 1) // width == last // width:
                F.add([last + 1], prev, w)
                prev = -1
                continue
        pick, t = {3, 7}, 0
        while len(pick) < 11:
            pick.add(others[(i * 9 + 5 * t) % len(others)])
            t += 1
        ids = []
        for b in sorted(pick):
            ids.append(b * width + (i + b) % (width - 2))
            if b in (3, 7) or (i + b) % 6 == 0:
                ids.append(b * width + (i + b) % (width - 2) + 1)
        prev = F.add(ids, -1, w)
    lone = list(range(24, 40))
    for i in range(70):
        pick, t = {3}, 0
        while len(pick) < 11:
            pick.add(lone[(i * 3 + 3 * t + t // 11) % len(lone)])
            t += 1
        F.add([b * width + (2 * i + b) % width for b in sorted(pick)], -1, JOIN_WEIGHTS[(i + 3) % len(JOIN_WEIGHTS)])
    return F.pat()


def stream_forest(n_roots=17000, wide=False, width=32):
    """n_roots two-block roots over N = 96, two ids in block 0 and one in block 1: stream (1, 0) holds exactly one record each (weights 1 ..
    127, one digit).  A few weights of 128 and more sit on one-block roots of block 2 (they widen the weight field of every record and add
    nothing to stream (1, 0)).  wide: a few nodes over the blocks 0, 2 and 3 (N = 128), which add nothing to it either."""
    F = V._Forest()
    for i in range(n_roots):
        a = i % (width - 1)
        b = a + 1 + (i // width) % (width - 1 - a)
        F.add([a, b, width + (i * 7) % width], -1, 1 + i % 127)
    for j, w in enumerate((128, 255, 16384, (1 << 32) - 1)):
        F.add([2 * width + j, 2 * width + j + 5], -1, w)
    if wide:
        for j in range(5):
            r = F.add([j, 2 * width + 9 + j, 3 * width + j], -1, 1 + j)
            F.add([3 * width + 10 + j, 3 * width + 20 + j] if j % 2 else [3 * width + 10 + j], r, 127 + j)
    return F.pat()


BOUNDARY_N = (2016, 2017, 8192, 8193)                          # 63 | 64 blocks: few streams | row mode; 256 | 257 blocks: second level | none


# ------------------------------------------------------------------------------------------------------------------------------------
# census
# ------------------------------------------------------------------------------------------------------------------------------------
def preorder(par):
    """DFS pre-order of a forest: roots ascending, children in ascending pattern id"""
    P = len(par)
    kids = [[] for _ in range(P)]
    roots = []
    for p in range(P):
        (kids[par[p]] if par[p] >= 0 else roots).append(p)
    order, stack = [], roots[::-1]
    while stack:
        p = stack.pop()
        order.append(p)
        stack.extend(kids[p][::-1])
    assert len(order) == P
    return order


def census(pat, width, run_nodes=256, l2_min=L2_MIN_DEFAULT):
    """What the wide-node kernel and the second level are given, counted on the host from the forest alone.

    Per node: blocks of its full list (nb), own pairs (distinct blocks of its local ids), first own block, whether that is the parent's last
    block (seam), the records it owns (block pairs a >= b, a diagonal pair only with two ids or more in the block; none without a weight).
    The wide list = the nodes with nb > 2 in pre-order; position // 64 is the batch, position // run_nodes the run.  A wide node's parent
    list comes from NONE (a root), FN1 / FN2 (a parent of one / two blocks), LANE (a wide parent in the batch) or the CHAIN (a wide parent
    before the batch: in the same run, or in an earlier run — then the chain was rebuilt at the run's start)."""
    par, w = pat["parent"].numpy(), pat["num_kmers"].numpy()
    lp, ids = pat["local_ptr"].numpy(), pat["local_ids"].numpy()
    P = len(par)
    blks, last_blk, cnt = [None] * P, [-1] * P, [None] * P
    npairs, b0, nl = [0] * P, [-1] * P, [0] * P
    for p in range(P):
        loc = ids[lp[p]: lp[p + 1]] // width
        own, oc = np.unique(loc, return_counts=True)
        base = dict(cnt[par[p]]) if par[p] >= 0 else {}
        for b, c in zip(own.tolist(), oc.tolist()):
            base[b] = base.get(b, 0) + c
        cnt[p] = base
        blks[p] = len(base)
        last_blk[p] = max(base) if base else -1
        npairs[p], b0[p] = len(own), (int(own[0]) if len(own) else -1)
        nl[p] = (nl[par[p]] if par[p] >= 0 else 0) + len(loc)
    acting = [bool(w[p] != 0 and nl[p] >= 2) for p in range(P)]
    records = [blks[p] * (blks[p] - 1) // 2 + sum(1 for c in cnt[p].values() if c >= 2) if acting[p] else 0 for p in range(P)]
    order = preorder(par.tolist())
    wide = [p for p in order if blks[p] > 2]
    pos = {p: k for k, p in enumerate(wide)}
    res = {"n_wide": len(wide), "n_records": int(sum(records)), "n_wide_records": int(sum(records[p] for p in wide)),
           "n_joined": sum(1 for p in wide if acting[p] and blks[p] >= l2_min), "nodes": P,
           "acting_blocks": {}, "classes": {}, "single_id_diagonals": 0}
    for p in wide:
        if acting[p]:
            res["acting_blocks"][blks[p]] = res["acting_blocks"].get(blks[p], 0) + 1
            res["single_id_diagonals"] += sum(1 for c in cnt[p].values() if c == 1)
    src = {}
    for p in wide:
        k, q = pos[p], par[p]
        if q < 0:
            s = "NONE"
        elif blks[q] <= 2:
            s = "FN%d" % blks[q]
        elif pos[q] >= k // WAVE * WAVE:
            s = "LANE"
        else:
            s = "CHAIN_SAME_RUN" if pos[q] // run_nodes == k // run_nodes else "CHAIN_EARLIER_RUN"
        src[p] = s
        seam = q >= 0 and b0[p] == last_blk[q]
        key = (blks[p], s, bool(seam), min(npairs[p], 5))
        res["classes"][key] = res["classes"].get(key, 0) + 1
    # batches
    batches = []
    for k0 in range(0, len(wide), WAVE):
        lanes = wide[k0: k0 + WAVE]
        ox = [max(npairs[p] - 1, 0) for p in lanes]
        incl = np.cumsum(ox).tolist()
        top, rows, walks_memory = [], 0, 0
        for j, p in enumerate(lanes):
            t, through_memory = p, False
            while src[t] == "LANE":
                t = par[t]
                tj = pos[t] - k0
                through_memory = through_memory or (ox[tj] > 0 and incl[tj] > K1W_OXCAP)
            top.append(t)
            walks_memory += through_memory
            pre = blks[par[t]] - 1 if src[t].startswith("CHAIN") else 0
            if acting[p] or j == len(lanes) - 1:
                rows += blks[p] - pre
        light = [acting[p] and blks[p] < K1W_HEAVY for p in lanes]
        gaps = sum(1 for j in range(1, len(lanes) - 1) if not light[j] and any(light[:j]) and any(light[j + 1:]))
        batches.append({"first": k0, "lanes": len(lanes), "ox": int(sum(ox)), "rows": rows, "walks_memory": walks_memory,
                        "all_acting_narrow_based": len(lanes) == WAVE and all(acting[p] for p in lanes) and all(src[t] in ("NONE", "FN1", "FN2") for t in top),
                        "owners_without_records_between_owners": gaps})
    res["batches"] = batches
    # a wide parent at lane 63 with its child at lane 0 of the next batch / of the next run
    res["child_at_lane0_of_parent_at_lane63"] = sum(1 for p in wide if pos[p] % WAVE == 0 and par[p] >= 0 and pos.get(par[p], -9) == pos[p] - 1)
    res["child_at_run_start_of_parent_at_run_end"] = sum(1 for p in wide if pos[p] % run_nodes == 0 and par[p] >= 0 and pos.get(par[p], -9) == pos[p] - 1)
    # the root path of every run's first node: narrow ancestors first, then wide ones
    res["run_starts"] = []
    for k0 in range(0, len(wide), run_nodes):
        q, narrow, wides = par[wide[k0]], 0, 0
        while q >= 0:
            narrow += blks[q] <= 2
            wides += blks[q] > 2
            q = par[q]
        res["run_starts"].append((narrow, wides))
    return res


def stream_census(pat, width):
    """records per stream (block pair a >= b) of the acting nodes, one per node and pair (weights of one digit), and per block row a"""
    w = pat["num_kmers"].numpy()
    streams, rows = {}, {}
    for p, full in enumerate(V.full_lists(pat)):
        if w[p] == 0 or full.size < 2:
            continue
        b, c = np.unique(full // width, return_counts=True)
        for i in range(len(b)):
            for j in range(i + 1):
                if i != j or c[i] >= 2:
                    streams[(int(b[i]), int(b[j]))] = streams.get((int(b[i]), int(b[j])), 0) + 1
                    rows[int(b[i])] = rows.get(int(b[i]), 0) + 1
    return streams, rows


def join_census(pat, width):
    """per tile (block pair) the acting nodes of K1W_HEAVY blocks or more that hold both blocks; cells whose exact sum passes 2^32"""
    w = pat["num_kmers"].numpy()
    tiles = {}
    for p, full in enumerate(V.full_lists(pat)):
        if w[p] == 0 or full.size < 2:
            continue
        b = np.unique(full // width).tolist()
        if len(b) < K1W_HEAVY:
            continue
        for i in range(len(b)):
            for j in range(i + 1):
                tiles[(b[i], b[j])] = tiles.get((b[i], b[j]), 0) + 1
    return tiles


@functools.lru_cache(maxsize=None)
def case(name, *args):
    """forest, sample count and definition of a named case: computed once per process, shared, never written to"""
    if name == "wide":                                         # (width, light)
        width, light = args
        N = 35 * width + 1
        pat = wide_forest(N, width, "full", light)
    elif name == "boundary":                                   # (N,)
        width, N = 32, args[0]
        pat = wide_forest(N, width, "small")
    elif name == "join":
        width, N = 32, 40 * 32
        pat = join_forest(width)
    elif name == "stream":                                     # (roots, wide)
        width, N = 32, 128 if args[1] else 96
        pat = stream_forest(args[0], args[1], width)
    else:
        raise KeyError(name)
    exp = V.definition(pat, N)
    exp.setflags(write=False)
    return {"pat": pat, "N": N, "width": width, "exp": exp, "sparse": V.sparse_rows(exp, N)}


@functools.lru_cache(maxsize=None)
def census_of(name, args, run_nodes, l2_min):
    c = case(name, *args)
    return census(c["pat"], c["width"], run_nodes, l2_min)
