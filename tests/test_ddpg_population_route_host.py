"""agents.ddpg_population_route: which way every agent of a DDPGPopulation trains and which groups its launches take,
decided from per-agent facts and the library's own ssc_ddpg_learner_path -- so none of this needs a GPU.  The array
addresses are made up: the route only compares them.  Every expectation is the one tests/test_gpu_ddpg_many*.py assert
on real agents, or follows from the rule in the route's docstring."""
import ctypes

import pytest

from tests.test_ddpg_layout_host import _desc

SHIPPED = ((64, 32), None)
MIXED = [((64, 32), None), ((128, 64), None), ((64, 32), None), ((200, 100), (128, 64))]   # tests/test_gpu_ddpg_many_wide.py
ONE, WIDE, POP, ALONE = "one_workgroup", "wide", "wide_popart", "alone"


@pytest.fixture(scope="module")
def agents_mod():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi, agents
    _ffi.lib()
    return agents


@pytest.fixture(autouse=True)
def _defaults(agents_mod, monkeypatch):
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)
    monkeypatch.setattr(agents_mod, "POPULATION_GROUPED_WIDE", True)
    monkeypatch.setattr(agents_mod, "POPULATION_WIDE_MIN_GROUP", 2)
    monkeypatch.setattr(agents_mod, "POPULATION_POPART_MIN_GROUP", 2)


def facts(shapes, popart=(), stats=(), shared=None, **kw):
    """agent p: actor / critic shapes[p] at batch 64, Pop-Art if p in popart, statistics if p in stats; ``shared`` = (p, q):
    agent q's critic is agent p's"""
    out = []
    for p, (actor, critic) in enumerate(shapes):
        arrays = [0x1000_0000 * (p + 1) + 0x10_0000 * k for k in range(9)]
        if shared is not None and p == shared[1]:
            arrays[1] = 0x1000_0000 * (shared[0] + 1) + 0x10_0000
        out.append((_desc(h=actor, critic_h=critic, **kw), p in popart, p in stats, tuple(arrays)))
    return out


def route(agents_mod, f):
    ways, groups = agents_mod.ddpg_population_route(f)
    assert sorted(p for _, ps in groups for p in ps) == [p for p, w in enumerate(ways) if w != ALONE]
    assert all(ways[p] == way for way, ps in groups for p in ps)
    return ways, groups


def fused(groups, P):
    """what DDPGPopulation.fused says of these groups"""
    return groups == [(ONE, list(range(P)))]


def test_shipped_population_is_fused(agents_mod):
    ways, groups = route(agents_mod, facts([SHIPPED] * 4))
    assert ways == (ONE,) * 4 and fused(groups, 4)
    ways, groups = route(agents_mod, facts([SHIPPED] * 4, stats=range(4)))
    assert ways == (ONE,) * 4 and fused(groups, 4)


def test_statistics_on_one_agent_make_a_group_of_its_own(agents_mod):
    ways, groups = route(agents_mod, facts([SHIPPED] * 4, stats=[3]))
    assert ways == (ONE,) * 4 and groups == [(ONE, [0, 1, 2]), (ONE, [3])] and not fused(groups, 4)
    ways, groups = route(agents_mod, facts([SHIPPED] * 4, stats=[1], obs=3))
    assert groups == [(ONE, [0, 2, 3]), (ONE, [1])]


def test_mixed_shapes(agents_mod):
    ways, groups = route(agents_mod, facts(MIXED))
    assert ways == (ONE, WIDE, ONE, WIDE) and groups == [(ONE, [0, 2]), (WIDE, [1, 3])] and not fused(groups, 4)


def test_a_lone_wide_agent_trains_alone(agents_mod):
    ways, groups = route(agents_mod, facts([SHIPPED, ((128, 64), None), SHIPPED, SHIPPED]))
    assert ways == (ONE, ALONE, ONE, ONE) and groups == [(ONE, [0, 2, 3])] and not fused(groups, 4)


def test_popart_agents(agents_mod):
    wide = ((128, 64), None)
    ways, groups = route(agents_mod, facts([wide] * 4, popart=[1]))
    assert ways == (WIDE, ALONE, WIDE, WIDE) and groups == [(WIDE, [0, 2, 3])]
    ways, groups = route(agents_mod, facts([wide, SHIPPED, wide, ((200, 100), None)], popart=[1, 2]))
    assert ways == (WIDE, POP, POP, WIDE) and groups == [(WIDE, [0, 3]), (POP, [1, 2])]
    ways, groups = route(agents_mod, facts(MIXED, popart=range(4)))
    assert ways == (POP,) * 4 and groups == [(POP, [0, 1, 2, 3])] and not fused(groups, 4)


def test_path_switches(agents_mod, monkeypatch):
    monkeypatch.setenv("SSC_DDPG_WIDE", "1")
    ways, groups = route(agents_mod, facts([SHIPPED] * 4))
    assert ways == (WIDE,) * 4 and groups == [(WIDE, [0, 1, 2, 3])]
    monkeypatch.delenv("SSC_DDPG_WIDE")
    monkeypatch.setenv("SSC_DDPG_INTERPRETER", "1")              # the step interpreter: no grouped launch serves it
    assert route(agents_mod, facts([SHIPPED] * 4)) == ((ALONE,) * 4, [])
    monkeypatch.setenv("SSC_DDPG_INTERPRETER", "0")
    assert fused(route(agents_mod, facts([SHIPPED] * 4))[1], 4)


@pytest.mark.parametrize("case", ["mixed", "wide_switch", "statistics", "popart"])
def test_switch_off_leaves_only_the_uniform_launch(agents_mod, monkeypatch, case):
    monkeypatch.setattr(agents_mod, "POPULATION_GROUPED_WIDE", False)
    if case == "wide_switch":
        monkeypatch.setenv("SSC_DDPG_WIDE", "1")
    f = dict(mixed=lambda: facts(MIXED), wide_switch=lambda: facts([SHIPPED] * 4), popart=lambda: facts(MIXED, popart=range(4)),
             statistics=lambda: facts([((128, 64), None)] * 4, stats=[3]))[case]()
    assert route(agents_mod, f) == ((ALONE,) * 4, [])
    assert route(agents_mod, facts([SHIPPED] * 4, stats=[3])) == ((ALONE,) * 4, [])
    if case != "wide_switch":
        ways, groups = route(agents_mod, facts([SHIPPED] * 4))
        assert ways == (ONE,) * 4 and fused(groups, 4)


def test_a_shared_array_sends_every_agent_alone(agents_mod):
    assert route(agents_mod, facts([SHIPPED] * 4, shared=(0, 2))) == ((ALONE,) * 4, [])
    assert route(agents_mod, facts(MIXED, shared=(1, 3))) == ((ALONE,) * 4, [])


def test_minimum_group_sizes(agents_mod, monkeypatch):
    monkeypatch.setattr(agents_mod, "POPULATION_WIDE_MIN_GROUP", 3)
    monkeypatch.setattr(agents_mod, "POPULATION_POPART_MIN_GROUP", 3)
    ways, groups = route(agents_mod, facts(MIXED))
    assert ways == (ONE, ALONE, ONE, ALONE) and groups == [(ONE, [0, 2])]
    wide = ((128, 64), None)
    ways, groups = route(agents_mod, facts([wide] * 4, popart=[1, 2]))
    assert ways == (ALONE,) * 4 and groups == []
    ways, groups = route(agents_mod, facts([wide] * 5, popart=[1, 2, 4]))
    assert ways == (ALONE, POP, POP, ALONE, POP) and groups == [(POP, [1, 2, 4])]
    ways, groups = route(agents_mod, facts([SHIPPED] * 4 + [wide] * 3, stats=[3]))      # one-workgroup groups of any size
    assert ways == (ONE,) * 4 + (WIDE,) * 3 and groups == [(ONE, [0, 1, 2]), (ONE, [3]), (WIDE, [4, 5, 6])]


def test_a_regularisation_that_rounds_to_zero_goes_where_the_library_says(agents_mod):
    """critic_l2_reg = 1e-46 is 0.0f in the descriptor: the library calls the shape the shipped one, and so does the route"""
    from smartstartcontinuous_amd import _ffi
    f = facts([SHIPPED] * 4, critic_l2_reg=1e-46)
    assert f[0][0].critic_l2_reg == 0.0
    assert _ffi.lib().ssc_ddpg_learner_path(ctypes.byref(f[0][0]), 1, 0) == _ffi.SSC_DDPG_PATH_FIXED
    ways, groups = route(agents_mod, f)
    assert ways == (ONE,) * 4 and fused(groups, 4)
    f = facts([SHIPPED] * 4, critic_l2_reg=1e-2)
    assert route(agents_mod, f) == ((WIDE,) * 4, [(WIDE, [0, 1, 2, 3])])
