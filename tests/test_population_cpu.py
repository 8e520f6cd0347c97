"""CPU-side checks of the population entry points (include/rdis_hip.h, "populations"): the library exports them, the
Python binding covers them, and NULL handles are rejected without touching a device."""
from rdis_amd import capi

NAMES = ("rdis_hip_population_create", "rdis_hip_population_destroy", "rdis_hip_population_set_x", "rdis_hip_population_get_x",
         "rdis_hip_population_assign", "rdis_hip_population_eval", "rdis_hip_plan_solve_population", "rdis_hip_plan_fetch_population")


def test_population_symbols_load():
    lib = capi.load_library()
    for n in NAMES:
        assert n in capi.SYMBOLS and getattr(lib, n) is not None
    for n in ("set_x", "get_x", "assign", "eval", "close"):
        assert callable(getattr(capi.Population, n))
    assert callable(capi.Plan.solve_population) and callable(capi.Plan.fetch_population)


def test_null_arguments_are_rejected():
    lib = capi.load_library()
    assert lib.rdis_hip_population_create(None, 1, None, None) == -1
    assert lib.rdis_hip_plan_solve_population(None, None, 10, 1e-8) == -1
    assert lib.rdis_hip_population_eval(None, 0, None, None) == -1
    assert lib.rdis_hip_population_set_x(None, 0, 0, 0, None, None) == -1
    assert lib.rdis_hip_population_get_x(None, 0, 0, 0, None, None) == -1
    assert lib.rdis_hip_population_assign(None, 0) == -1
    assert lib.rdis_hip_plan_fetch_population(None, None, None, None, None, None, None, None) == -1
    lib.rdis_hip_population_destroy(None)
