"""rdis_amd/csrc/replica_layout.hpp -- the replicas of the five many-member entries (rdis_hip_plan_solve_starts,
rdis_hip_plan_solve_population, rdis_hip_population_eval, both forms of rdis_hip_population_eval_grad) described once -- without a
GPU: tests/cpp/replica_layout_test.cpp checks the layouts' properties over a grid of arguments (parts in declaration order, no
overlap, multiples of 8 bytes, the last part ends at R * member_bytes(), a part of zero bytes moves nothing) and
members_per_launch against the four rules it replaced; here every size, offset and stride it prints is compared with the
expression the entry itself had before the layouts were described in one place, written out again as literal arithmetic: the
addresses the kernels are handed, relative to their buffer, have not moved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = (1, 2, 65535)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("replica_layout") / "replica_layout_test")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "replica_layout_test.cpp")],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr          # (the program's own checks of the properties)
    rows = out.stdout.splitlines()
    assert rows[-1] == "ok"
    return rows[:-1]


def cases(lines, tag):
    got = [tuple(int(t) for t in ln.split()[1:]) for ln in lines if ln.split()[0] == tag]
    assert got
    return got


def test_every_line_is_compared(lines):
    assert {ln.split()[0] for ln in lines} == {"starts", "population", "ptm", "eval", "gradf", "gradl", "members"}


def test_multi_start(lines):
    """rdis_hip_plan_solve_starts: work_doubles = 5 nfree + ngfac + (plain ? N : 0) and dir_doubles = plain ? N : 0, both charged;
    ms_work of R work_doubles, ms_dir of R dir_doubles; S.gfac = S.ws + R 5 nfree, S.x = S.gfac + R ngfac"""
    seen = set()
    for nfree, ngfac, plain, N, R, member, total, ws, gfac, x, dir_member, dir_total, charged in cases(lines, "starts"):
        work_doubles = 5 * nfree + ngfac + (N if plain else 0)
        dir_doubles = N if plain else 0
        assert (member, total) == (work_doubles * 8, R * work_doubles * 8)
        assert (dir_member, dir_total) == (dir_doubles * 8, R * dir_doubles * 8)
        assert charged == (work_doubles + dir_doubles) * 8
        assert (ws, gfac, x) == (0, 8 * R * 5 * nfree, 8 * (R * 5 * nfree + R * ngfac))
        seen.add((bool(plain), R))
    assert seen == {(pl, R) for pl in (False, True) for R in LAUNCHES}     # x present and absent, at every launch size


def test_population_solve(lines):
    """solve_population_range: work_doubles = nlisted > 0 ? 5 nfree + ngfac : 0, rot_doubles = tiny_records ? N : 0,
    dir_doubles = plain ? N : 0; ms_work of R (work_doubles + rot_doubles); S.gfac = S.ws + R (work_doubles ? 5 nfree : 0),
    XR = S.ws + R work_doubles"""
    seen = set()
    for listed, nfree, ngfac, records, plain, N, R, member, total, ws, gfac, rot, dir_member, dir_total in cases(lines, "population"):
        work_doubles = 5 * nfree + ngfac if listed else 0
        rot_doubles = N if records else 0
        dir_doubles = N if plain else 0
        assert (member, total) == ((work_doubles + rot_doubles) * 8, R * (work_doubles + rot_doubles) * 8)
        assert (dir_member, dir_total) == (dir_doubles * 8, R * dir_doubles * 8)
        assert (ws, gfac, rot) == (0, 8 * R * (5 * nfree if work_doubles else 0), 8 * R * work_doubles)
        seen.add((bool(listed), bool(records), R))
    assert seen >= {(li, rec, R) for li in (False, True) for rec in (False, True) for R in LAUNCHES}
    # no blocks beside an LDS-resident part (tests/cpp/population_ptm_replica_test.cpp): 8 (5 100 + 7)
    assert any(c[:6] == (1, 100, 7, 0, 0, 0) and c[7] == 8 * 507 for c in cases(lines, "population"))


def test_point_major(lines):
    """solve_population_range: ptm_bytes = blocks (6 + 6 + 6) 8 + (blocks > 0 ? cptr_len 32 : 0); plane = R PT_REC blocks doubles,
    RP.gh = RP.rec + plane, RP.bex = RP.gh + plane, RP.cbox = (float*)(RP.bex + plane)"""
    got = cases(lines, "ptm")
    for blocks, cptr_len, R, member, total, rec, gh, bex, cbox in got:
        ptm_bytes = blocks * (6 + 6 + 6) * 8 + (cptr_len * 32 if blocks > 0 else 0)
        plane = R * 6 * blocks
        assert (member, total) == (ptm_bytes, R * ptm_bytes)
        assert (rec, gh, bex, cbox) == (0, 8 * plane, 8 * 2 * plane, 8 * 3 * plane)
    # the replica tests/test_gpu_population_ptm.py measures through device_bytes(): 200 point blocks, five chunk-table entries
    assert (200, 5, 1, 28960, 28960, 0, 9600, 19200, 28800) in got and 200 * (6 + 6 + 6) * 8 + 5 * 32 == 28960
    assert (0, 5, 2, 0, 0, 0, 0, 0, 0) in got                              # a plan without point blocks: nothing


def test_evaluation(lines):
    """population_eval_enqueue: eval_partial of R per doubles, eval_xr of R N doubles on the records branch; the budget is charged
    8 (max(per, 1) + (records ? N : 0))"""
    seen = set()
    for per, N, records, R, part_member, part_total, xr_member, xr_total, charged in cases(lines, "eval"):
        assert (part_member, part_total) == (per * 8, R * per * 8)
        assert (xr_member, xr_total) == ((N * 8, R * N * 8) if records else (0, 0))
        assert charged == 8 * (max(per, 1) + (N if records else 0))
        seen.add((bool(records), R))
    assert seen == {(rec, R) for rec in (False, True) for R in LAUNCHES}


def test_gradient_fused(lines):
    """population_grad_enqueue, fused: camrec_stride = GRAD_REC ncam_blocks, cstage_stride = 9 max(cstage_slots, 1), pstage_stride =
    3 max(pstage_slots, 1), partial_stride = nchunks (at least 1 on this branch); camrec = W, cstage = camrec + R camrec_stride,
    pstage = cstage + R cstage_stride, partial = pstage + R pstage_stride; grad_ws of R grad_member_bytes"""
    got = cases(lines, "gradf")
    for ncb, cs, ps, nch, R, member, total, camrec, cstage, pstage, partial, s_cam, s_cs, s_ps, s_part in got:
        assert nch >= 1
        strides = (14 * ncb, 9 * max(cs, 1), 3 * max(ps, 1), nch)
        assert (s_cam, s_cs, s_ps, s_part) == strides
        assert member == 8 * (14 * ncb + 9 * max(cs, 1) + 3 * max(ps, 1) + max(nch, 1)) and total == R * member
        assert (camrec, cstage, pstage, partial) == (0, 8 * R * strides[0], 8 * (R * strides[0] + R * strides[1]),
                                                     8 * (R * strides[0] + R * strides[1] + R * strides[2]))
    # the pinned member: 49 camera blocks, 10 camera slots, 20 point slots, 63 chunks
    assert any(c[:4] == (49, 10, 20, 63) and c[5] == 7192 for c in got) and 8 * (686 + 90 + 60 + 63) == 7192
    assert any(c[:4] == (5, 0, 0, 1) and c[5] == 8 * (70 + 9 + 3 + 1) for c in got)     # no staged block: each array one slot
    assert any(c[0] == 0 for c in got)                                                  # no camera records


def test_gradient_short_and_two_pass(lines):
    """population_grad_enqueue, short and two-pass: gfac = W, part = W + R nslots, gfac's stride nslots; grad_ws of
    R 8 (nslots + 1) and R 8 (nslots + max(blocks, 1))"""
    got = cases(lines, "gradl")
    for nslots, blocks, R, member, total, gfac, part, stride in got:
        assert blocks >= 1
        assert (member, total) == (8 * (nslots + blocks), R * 8 * (nslots + blocks))
        assert (gfac, part, stride) == (0, 8 * R * nslots, nslots)
    # full ladybug on the two-pass form: twelve partials a factor and 125 block sums
    assert any(c[:2] == (382116, 125) and c[3] == 8 * 382241 for c in got)
    assert any(c[0] == 0 for c in got)


def test_members_per_launch(lines):
    """the four rules as they stood: the multi-start entry's inline one, population_members_per_launch, eval_members_per_launch
    (its bytes: at least 8) and grad_members_per_launch (asked only with bytes of at least 8)"""
    got = cases(lines, "members")
    assert len(got) >= 28
    for count, budget, per, R in got:
        starts = min(min(max(1, budget // per) if per else count, count), 65535)
        population = min(min(max(1, budget // per) if per > 0 else count, count), 65535)
        assert R == starts == population >= 1, (count, budget, per, R)
        if per >= 8:
            evaluation = max(1, min(min(count, 65535), max(1, budget // per)))
            gradient = max(1, min(min(count, 65535), max(1, budget // max(per, 1))))
            assert R == evaluation == gradient, (count, budget, per, R)
    # what the three programs beside this one print
    for case in [(5, 17980, 7192, 2), (5, 1, 7192, 1), (3, 0, 7192, 1), (100000, 1 << 30, 8, 65535), (70000, 1 << 40, 7192, 65535),
                 (256, 1 << 30, 3056936, 256), (1000, 1 << 30, 3056936, (1 << 30) // 3056936), (5, 72400, 28960, 2), (7, 12345, 0, 7),
                 (256, 1 << 28, 1123680, (1 << 28) // 1123680), (5, 2 * 8 * 23832, 8 * 23832, 2), (5, 2 * 8 * 23832 - 1, 8 * 23832, 1),
                 (5, 1024, 504, 1024 // 504), (5, 1023, 504, 1023 // 504), (1, 0, 8, 1), (1000000, 1 << 30, 8, 65535),
                 (256, 1 << 30, 8 * 136, 256)]:
        assert case in got, case
