"""rdis_amd/csrc/grad_tables.hpp -- a factor list's tables for the fused gradient (grad_fused.hpp: GradTables) -- without a GPU.
tests/cpp/grad_tables_test.cpp prints the tables of the cases given here; walk() then goes through them as grad_fused.hip's
kernels do -- rows by rc / rp, segment sums per chunk, cameras accumulated over a tile's chunks, straight or staged destinations,
the combine pass over cs_ptr / ps_ptr -- but carries sequences of list positions where the kernels carry doubles.  What reaches a
block's gradient entries must be exactly its listed factors in list order: that is the order of the sums."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ENTRY = 0xFFFF
PARTS = ("ptv", "tile_chunk0", "tile_cam0", "tile_cam", "chunk_cseg0", "cseg", "chunk_pseg0", "pseg", "cs_var", "cs_ptr", "ps_var", "ps_ptr", "zvar")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("grad_tables") / "grad_tables_test")
    subprocess.check_call([hipcc, "-x", "c++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "grad_tables_test.cpp")],
                          stderr=subprocess.DEVNULL)
    return out


class Case:
    """ncam camera blocks of 9 from 0, npt point blocks of 3 behind them, two variables in no block; factor i reads camera
    cams[i] and point pts[i]; the list is fac (None: all factors in order)"""

    def __init__(self, ncam, npt, cams, pts, fac=None, GW=512, tile_chunks=8, cam_soft=192):
        self.cam = 9 * np.asarray(cams, dtype=np.int64)
        self.pt = 9 * ncam + 3 * np.asarray(pts, dtype=np.int64)
        self.N = 9 * ncam + 3 * npt + 2
        blocks = np.unique(self.cam)                      # the camera blocks some factor of the PROBLEM reads, ascending
        self.ncb = len(blocks)
        self.cam_ord = np.full(self.N, -1, dtype=np.int64)
        self.cam_ord[blocks] = np.arange(self.ncb)
        self.fac = None if fac is None else np.asarray(fac, dtype=np.int64)
        self.nf = len(self.cam) if fac is None else len(self.fac)
        self.GW, self.tile_chunks, self.cam_soft = GW, tile_chunks, cam_soft

    def text(self):
        j = lambda a: " ".join(str(int(x)) for x in a)
        return "case %d %d %d %d %d %d %s %s %s %d %s\n" % (self.N, self.ncb, self.GW, self.tile_chunks, self.cam_soft, len(self.cam), j(self.cam),
                                                          j(self.pt), j(self.cam_ord), self.nf, "-1" if self.fac is None else "%d %s" % (self.nf, j(self.fac)))


def run(exe, cases):
    out = subprocess.run([exe], input="".join(c.text() for c in cases), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr          # (the program's own checks of the blocks' sizes)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == 5 * len(cases) + 1
    tables = []
    for k in range(len(cases)):
        chunk = lines[5 * k:5 * k + 5]
        assert chunk[4] == "end"
        tables.append({ln.split()[0]: np.array(ln.split()[1:], dtype=np.int64) for ln in chunk[:4]})
    return tables


def split(case, T):
    """the int32 block's parts by their offsets, each of the length the scalars say and padded to an even one with a zero"""
    nchunks, ntiles, _, ncs, nps, nz, _, _, npad = (int(x) for x in T["scalars"])
    blk, off = T["blk"], [int(x) for x in T["offsets"]] + [len(T["blk"])]
    parts = {}

    def take(i, n):
        assert off[i + 1] - off[i] == n + (n & 1), (PARTS[i], n)
        assert n % 2 == 0 or blk[off[i] + n] == 0
        parts[PARTS[i]] = [int(x) for x in blk[off[i]:off[i] + n]]
        return parts[PARTS[i]]

    assert off[0] == 0
    take(0, npad)
    assert take(1, ntiles + 1)[0] == 0
    ncam_entries = take(2, ntiles + 1)[-1]
    take(3, 2 * ncam_entries)
    take(5, 2 * take(4, nchunks + 1)[-1])
    take(7, 2 * take(6, nchunks + 1)[-1])
    take(8, ncs); take(9, ncs + 1); take(10, nps); take(11, nps + 1); take(12, nz)
    for name in ("tile_cam", "cseg", "pseg"):
        parts[name] = list(zip(parts[name][0::2], parts[name][1::2]))
    assert npad == nchunks * case.GW and len(T["sh"]) == 3 * npad
    for k, name in enumerate(("cl", "rc", "rp")):
        parts[name] = [int(x) for x in T["sh"][k * npad:(k + 1) * npad]]
    return parts


def walk(case, T):
    GW, nf, N = case.GW, case.nf, case.N
    nchunks, ntiles, ncam_cap, ncs, nps, nz, cslots, pslots, npad = (int(x) for x in T["scalars"])
    P = split(case, T)
    fid = list(range(nf)) if case.fac is None else [int(f) for f in case.fac]
    cam_of = [int(case.cam[f]) for f in fid]          # per list position: the camera block, the point block
    pt_of = [int(case.pt[f]) for f in fid]
    assert nchunks == (nf + GW - 1) // GW
    # padding entries
    for name in ("cl", "rc", "rp"):
        assert all(x == NO_ENTRY for x in P[name][nf:]), name
    assert all(x == 0 for x in P["ptv"][nf:])

    straight = ({}, {})                                # destination block -> the sequence that reached it, cameras / points
    stage = ([None] * cslots, [None] * pslots)         # staging slot -> (block, sequence, the tile / chunk that wrote it)

    def deliver(side, dest, block, seq, when):
        if dest >= 0:
            assert dest == block and block not in straight[side], (side, dest, block)
            straight[side][block] = seq
        else:
            slot = ~dest
            assert 0 <= slot < len(stage[side]) and stage[side][slot] is None, (side, slot)
            stage[side][slot] = (block, seq, when)

    tc0, tm0 = P["tile_chunk0"], P["tile_cam0"]
    first_var = {int(case.cam_ord[v]): v for v in range(N) if case.cam_ord[v] >= 0}
    assert tc0[-1] == nchunks and tm0[0] == 0 and tm0[-1] == len(P["tile_cam"])
    most = 1
    for t in range(ntiles):
        assert 0 < tc0[t + 1] - tc0[t] <= case.tile_chunks
        cams = P["tile_cam"][tm0[t]:tm0[t + 1]]
        nc = len(cams)
        assert tm0[t + 1] >= tm0[t] and all(0 <= o < case.ncb for o, _ in cams)
        j_lo, j_hi = tc0[t] * GW, min(nf, tc0[t + 1] * GW)
        assert sorted(o for o, _ in cams) == sorted({int(case.cam_ord[c]) for c in cam_of[j_lo:j_hi]})     # the tile's distinct cameras, each once
        assert tc0[t + 1] - tc0[t] == 1 or nc <= case.cam_soft
        most = max(most, nc)
        acc = [[] for _ in range(nc)]
        for ch in range(tc0[t], tc0[t + 1]):
            j0, j1 = ch * GW, min(nf, ch * GW + GW)
            rows = j1 - j0
            assert rows > 0
            crow, prow = [None] * rows, [None] * rows
            for j in range(j0, j1):
                assert 0 <= P["cl"][j] < nc and cams[P["cl"][j]][0] == case.cam_ord[cam_of[j]] and P["ptv"][j] == pt_of[j]
                assert 0 <= P["rc"][j] < rows and crow[P["rc"][j]] is None and 0 <= P["rp"][j] < rows and prow[P["rp"][j]] is None
                crow[P["rc"][j]] = j
                prow[P["rp"][j]] = j
            for side, seg0, segs in ((0, P["chunk_cseg0"], P["cseg"]), (1, P["chunk_pseg0"], P["pseg"])):
                assert 0 <= seg0[ch] < seg0[ch + 1] <= len(segs)
                mine = segs[seg0[ch]:seg0[ch + 1]]
                assert mine[-1][1] == rows and mine[0][1] == 0          # the list ends with {-, rows}; the first segment starts at row 0
                blocks_seen = set()
                for (what, r0), (_, r1) in zip(mine[:-1], mine[1:]):
                    assert 0 <= r0 < r1 <= rows
                    if side == 0:
                        seq = crow[r0:r1]
                        assert 0 <= what < nc and all(P["cl"][j] == what for j in seq) and what not in blocks_seen
                        blocks_seen.add(what)
                        acc[what] += seq
                    else:
                        seq = prow[r0:r1]
                        q = pt_of[seq[0]]
                        assert all(pt_of[j] == q for j in seq) and q not in blocks_seen
                        blocks_seen.add(q)
                        deliver(1, what, q, seq, ch)
        for (o, dest), seq in zip(cams, acc):
            deliver(0, dest, first_var[o], seq, t)
    assert ncam_cap == most

    # the combine pass
    final = ({}, {})
    for side, var, ptr, n in ((0, P["cs_var"], P["cs_ptr"], ncs), (1, P["ps_var"], P["ps_ptr"], nps)):
        assert ptr[0] == 0 and ptr[-1] == len(stage[side]) and None not in stage[side] and len(set(var)) == n
        final[side].update(straight[side])
        for b in range(n):
            slots = stage[side][ptr[b]:ptr[b + 1]]
            assert len(slots) >= 2                                         # (one partial sum would have gone straight)
            assert all(s[0] == var[b] for s in slots) and var[b] not in straight[side]       # one route, never both
            assert all(a[2] < c[2] for a, c in zip(slots[:-1], slots[1:]))                   # consecutive slots in tile / chunk order
            final[side][var[b]] = [j for s in slots for j in s[1]]
    # every block's gradient entries: its listed factors, in list order, each once
    for side, of in ((0, cam_of), (1, pt_of)):
        want = {}
        for j, b in enumerate(of):
            want.setdefault(b, []).append(j)
        assert final[side] == want, side
    read = np.zeros(N, dtype=bool)
    for b in set(cam_of):
        read[b:b + 9] = True
    for b in set(pt_of):
        read[b:b + 3] = True
    assert P["zvar"] == [int(v) for v in np.flatnonzero(~read)]
    return P


def test_one_entry_past_a_chunk(exe):
    """nf = 513: two chunks, the second with one row; one tile holds both, so every camera goes straight, and point 170, whose
    three factors are the list's last, is the one staged block"""
    n = 513
    case = Case(5, 171, [j % 5 for j in range(n)], [j // 3 for j in range(n)])
    T, = run(exe, [case])
    P = walk(case, T)
    assert list(T["scalars"][:2]) == [2, 1] and T["scalars"][3] == 0 and T["scalars"][8] == 1024
    assert P["ps_var"] == [9 * 5 + 3 * 170] and P["ps_ptr"] == [0, 2]
    assert all(dest >= 0 for _, dest in P["tile_cam"])


def test_two_tiles(exe):
    """nf = 8 * 512 + 1 with tiles of 8 chunks: camera 0 is read in both tiles (staged, two slots), cameras 1 .. 8 only in the first
    (straight); camera 9 and the last points are read by no factor"""
    n = 8 * 512 + 1
    case = Case(10, 1400, [j % 9 for j in range(n - 1)] + [0], [j // 3 for j in range(n)])
    T, = run(exe, [case])
    P = walk(case, T)
    assert list(T["scalars"][:4]) == [9, 2, 9, 1] and P["cs_var"] == [0] and P["cs_ptr"] == [0, 2]
    assert P["tile_chunk0"] == [0, 8, 9] and P["tile_cam0"] == [0, 9, 10]
    assert [d for o, d in P["tile_cam"]] == [~0] + [9 * c for c in range(1, 9)] + [~1]
    assert set(range(81, 90)) <= set(P["zvar"])


def test_cameras_beyond_the_soft_limit(exe):
    """a list cycling through 300 cameras: a chunk alone may hold them, a second chunk may not join it -- every tile is one chunk and
    numbers the cameras afresh; and a chunk that would ADD cameras beyond the limit (150 + 100 new ones) is backed out, the ones it
    shares with the tile numbered again in the next"""
    n = 3 * 512
    cycling = Case(350, 40, [j % 300 for j in range(n)], [(j * 7) % 40 for j in range(n)])
    adding = Case(350, 40, [(j // 512) * 100 + j % 150 for j in range(n)], [(j * 7) % 40 for j in range(n)])
    fits = Case(350, 40, [(j // 512) * 20 + j % 150 for j in range(n)], [(j * 7) % 40 for j in range(n)])      # 150, 170, 190 cameras: one tile
    Tc, Ta, Tf = run(exe, [cycling, adding, fits])
    Pc, Pa, Pf = walk(cycling, Tc), walk(adding, Ta), walk(fits, Tf)
    assert list(Tc["scalars"][:3]) == [3, 3, 300] and Pc["tile_cam0"] == [0, 300, 600, 900]
    assert list(Ta["scalars"][:3]) == [3, 3, 150] and Pa["tile_cam0"] == [0, 150, 300, 450]
    assert sorted(o for o, _ in Pa["tile_cam"][150:300]) == list(range(100, 250))
    assert list(Tf["scalars"][:3]) == [3, 1, 190]


def test_a_point_block_across_a_chunk_boundary(exe):
    """point-major runs of three; point 170 has four factors at list positions 510 .. 513: it alone is staged, two slots"""
    pts = [q for q in range(170) for _ in range(3)] + [170] * 4 + [q for q in range(171, 360) for _ in range(3)]
    case = Case(7, 360, [(j * 5) % 7 for j in range(len(pts))], pts)
    T, = run(exe, [case])
    P = walk(case, T)
    assert case.nf > 1024 and P["ps_var"] == [9 * 7 + 3 * 170] and P["ps_ptr"] == [0, 2]
    assert sum(1 for d, _ in P["pseg"] if d < 0) == 2


def test_explicit_shuffled_and_partial_lists(exe):
    """fac == null gives the tables of the same list given explicitly; a shuffled list; a list that leaves cameras and points unread"""
    rng = np.random.RandomState(5)
    F = 1300
    cams, pts = [(j * 3) % 11 for j in range(F)], [j // 4 for j in range(F)]
    whole = Case(11, 330, cams, pts)
    explicit = Case(11, 330, cams, pts, fac=range(F))
    shuffled = Case(11, 330, cams, pts, fac=rng.permutation(F))
    partial = Case(11, 330, cams, pts, fac=[f for f in rng.permutation(F) if cams[f] not in (2, 7) and pts[f] % 5 != 1])
    Tw, Te, Ts, Tp = run(exe, [whole, explicit, shuffled, partial])
    for name in ("scalars", "offsets", "blk", "sh"):
        assert np.array_equal(Tw[name], Te[name]), name
    walk(whole, Tw)
    Ps, Pp = walk(shuffled, Ts), walk(partial, Tp)
    assert Ts["scalars"][4] > 100                                   # a shuffled list stages most of its points
    assert set(range(18, 27)) | set(range(63, 72)) | {9 * 11 + 3, 9 * 11 + 4, 9 * 11 + 5} <= set(Pp["zvar"])
    assert partial.ncb == 11 and sorted({o for o, _ in Pp["tile_cam"]}) == [0, 1, 3, 4, 5, 6, 8, 9, 10]     # ordinals of the PROBLEM's blocks


def test_random_lists_at_a_chunk_of_eight(exe):
    """chunks of 8, tiles of 2, at most 3 cameras in a tile of two chunks: 200 seeded lists over 6 cameras and 20 points -- at this
    width backed-out chunks, blocks across boundaries, single-row chunks and unread blocks occur in most lists"""
    rng = np.random.RandomState(20240607)
    cases = []
    for k in range(200):
        F = int(rng.randint(9, 70))
        ncam_used = int(rng.randint(1, 7))
        cams = rng.randint(0, ncam_used, size=F)
        pts = np.sort(rng.randint(0, 20, size=F)) if k % 3 == 0 else rng.randint(0, 20, size=F)      # a third of them point-major
        how = k % 4
        fac = None if how == 0 else rng.permutation(F) if how == 1 else rng.permutation(F)[:int(rng.randint(1, F + 1))] if how == 2 else \
            np.sort(rng.permutation(F)[:int(rng.randint(1, F + 1))])
        cases.append(Case(6, 20, cams, pts, fac=fac, GW=8, tile_chunks=2, cam_soft=3))
    tables = run(exe, cases)
    backed_out = staged_c = staged_p = 0
    for case, T in zip(cases, tables):
        P = walk(case, T)
        backed_out += any(b - a == 1 and a + 1 < T["scalars"][0] for a, b in zip(P["tile_chunk0"][:-1], P["tile_chunk0"][1:]))
        staged_c += T["scalars"][3] > 0
        staged_p += T["scalars"][4] > 0
    assert backed_out > 50 and staged_c > 50 and staged_p > 50
