"""The plan's options as a table (rdis_amd/csrc/plan_options.hpp), without a GPU.  ROWS restates what rdis_hip_plan_set_option did
with every option when it was an if / else chain -- the name, the field and its default, the values it took, one value it
refused on each side that has one, the message, whether the partition was marked dirty, what else the call did to the plan --
and tests/cpp/plan_options_test.cpp prints what plan_option_set does with those values; the two are compared with ==."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIG = 1 << 40          # (for the options without an upper bound)
SIZES = (0, 64, 128, 256, 512, 768, 1024)


def _row(name, default, accepted, refused, message, dirty=True, effects=(), field=None, flag=False):
    return dict(name=name, field=field or name, default=default, accepted=tuple(accepted), refused=tuple(refused), message=message, dirty=dirty,
                effects=list(effects), flag=flag)


def _flag(name, default, dirty=True, field=None):
    return _row(name, default, (0, 1, 7, -3), (), None, dirty=dirty, field=field, flag=True)


# name, default, (lowest and highest accepted value | the allowed set), (a refused value on each side that has one), message
ROWS = [
    _row("block_threads", 0, SIZES, (-64, 32, 2048), "block_threads must be 0, 64, 128, 256, 512, 768 or 1024"),
    _row("coop_min_factors", 4096, (0, BIG), (-1,), "coop_min_factors < 0"),
    _row("quad_min_components", 16384, (0, BIG), (-1,), "quad_min_components < 0"),
    _row("coop_group_min_factors", 256, (0, BIG), (-1,), "coop_group_min_factors < 0"),
    _row("tiny_max_blocks", 0, (0, 1 << 20), (-1, (1 << 20) + 1), "tiny_max_blocks out of range"),
    _flag("overlap_batch", 1),
    _row("row_min_components", 4096, (0, BIG), (-1,), "row_min_components < 0"),
    _row("camera_records", 1, (0, 2), (-1, 3), "camera_records must be 0, 1 or 2"),
    _row("quad_max_vars", 4, (0, 4), (-1, 5), "quad_max_vars out of range"),
    _row("coop_max_components", 48, (0, 4096), (-1, 4097), "coop_max_components out of range"),
    _row("coop_workgroups", 0, (0, 512), (-1, 513), "coop_workgroups out of range"),
    _row("coop_threads", 256, (128, 256, 512), (64, 192, 1024), "coop_threads must be 128, 256 or 512"),
    _flag("coop_speculate", 1),
    _flag("coop_pipeline", 1),
    _flag("lds_resident", 1),
    _row("ptm_stream", 1, (0, 2), (-1, 3),
         "ptm_stream must be 0 (never), 1 (components too large for the LDS) or 2 (every component its tables fit)"),
    _row("ptm_group", 0, (0, 512), (-1, 513),
         "ptm_group must be 0 (auto), 1 (never) or the number of workgroups per component (at most 16; up to 512 for the wide groups of a few "
         "large components)", dirty=False),
    _row("ptm_round_slots", 0, (0, 2), (-1, 3), "ptm_round_slots must be 0 (two where the LDS holds them), 1 or 2", dirty=False, effects=["rounds"]),
    _row("ptm_threads", 0, (0, 256, 512, 768), (-256, 128, 1024), "ptm_threads must be 0, 256, 512 or 768"),
    _row("ptm_local_cameras", -1, (-1, 1), (-2, 2),
         "ptm_local_cameras must be -1 (where a wide group's cameras do not fit the LDS), 0 (never) or 1 (every wide group)", effects=["local"]),
    _flag("emulate_stale_cache", 0, field="emulate_stale"),
    _row("factor_rounding", -1, (-1, 1), (-2, 2), "factor_rounding must be -1 (auto), 0 (fused multiply-adds) or 1 (the reference's rounding)"),
    _flag("lds_camera_sums", 1),
    _flag("lds_matrix", 0, dirty=False),
    _row("lds_rot", -1, (-1, 1), (-2, 2), "lds_rot must be -1, 0 or 1"),
    _row("lds_threads", 0, SIZES, (-64, 32, 2048), "lds_threads must be 0, 64, 128, 256, 512, 768 or 1024"),
    _flag("force_stream", 0),
    _row("coop_poll_delay", 16, (0, 1024), (-1, 1025), "coop_poll_delay out of range"),
    _row("coop_poll_inflight", 0, (0, 1), (-1, 2), "coop_poll_inflight must be 0 (one poll at a time) or 1 (a ring of polls in flight)"),
    _row("coop_poll_stagger", 2, (0, 64), (-1, 65), "coop_poll_stagger out of range (0 ... 64)"),
    _row("starts_workspace_bytes", 1 << 30, (0, 1 << 62), (-1,), "starts_workspace_bytes < 0", dirty=False, effects=["workspace"]),
    _flag("population_point_major", 0, dirty=False),
    _flag("population_plain", 0, dirty=False),
    _flag("population_tiny", 0, dirty=False),
    _row("tiny_population_fill", 1, (1, 64), (0, 65), "tiny_population_fill out of range (1 ... 64)", dirty=False),
    _row("trace_records", 0, (0, 1 << 22), (-1, (1 << 22) + 1), "trace_records out of range", effects=["trace"]),
    _row("dump_iters", 0, (0, 4096), (-1, 4097), "dump_iters out of range", effects=["dump"]),
]
CLEAN = {"ptm_group", "ptm_round_slots", "lds_matrix", "starts_workspace_bytes", "population_point_major", "population_plain", "population_tiny",
         "tiny_population_fill"}
UNKNOWN = "no_such_option"


def test_the_restated_table_is_whole():
    assert len(ROWS) == 37 and len({r["name"] for r in ROWS}) == 37 and len({r["field"] for r in ROWS}) == 37
    assert {r["name"] for r in ROWS if not r["dirty"]} == CLEAN
    for r in ROWS:
        assert r["flag"] or (r["refused"] and r["message"]), r["name"]
        assert any(v != r["default"] for v in r["accepted"]), r["name"]       # (a stored value shows as a changed field)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("plan_options") / "plan_options_test")
    # (for the host alone, as tests/test_population_select_cpu.py builds its program)
    subprocess.check_call([hipcc, "-x", "c++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_options_test.cpp")],
                          stderr=subprocess.DEVNULL)

    def ask(commands):
        run = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr
        got = [json.loads(ln) for ln in run.stdout.splitlines()]
        assert got[-1] == "ok" and len(got) == len(commands) + 1
        return got[:-1]
    return ask


def test_names_and_defaults(ask):
    names, defaults = ask(["names", "defaults"])
    assert sorted(names) == sorted(r["name"] for r in ROWS) and len(names) == 37
    assert defaults == {r["field"]: r["default"] for r in ROWS}


def test_every_row(ask):
    commands = [(r, v, True) for r in ROWS for v in r["accepted"]] + [(r, v, False) for r in ROWS for v in r["refused"]]
    answers = ask(["set %s %d" % (r["name"], v) for r, v, _ in commands])
    clean = set()
    for (r, v, accepted), got in zip(commands, answers):
        if not accepted:
            assert got == {"result": "refused", "message": r["message"], "changed": {}}, (r["name"], v)
            continue
        stored = (1 if v else 0) if r["flag"] else v
        want = {"result": "stored", "message": "(none)", "dirty": r["dirty"], "effects": r["effects"],
                "changed": {} if stored == r["default"] else {r["field"]: stored}}
        assert got == want, (r["name"], v)
        if not got["dirty"]:
            clean.add(r["name"])
    assert clean == CLEAN


def test_unknown_name_and_flag_given_seven(ask):
    unknown, seven = ask(["set %s 1" % UNKNOWN, "set lds_matrix 7"])
    assert unknown == {"result": "unknown", "message": "unknown option " + UNKNOWN, "changed": {}}
    assert seven["result"] == "stored" and seven["changed"] == {"lds_matrix": 1}
