"""The launch rule of the marched observers (observer_plan, ludvm_amd/csrc/plan_rule.hpp), asked of the header itself through
tools/plan_rule.py: the plans that tests/observer_sources_common.py's cases are built around, as values, and what every plan
must satisfy for a step never to outrun the slab its setter allocated.  No GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_rule  # noqa: E402

# (kind, count, ns_ub) -> (tiles, pad, chunk, nsplit): the values of the five per-observer rules this one replaced
TABLE = [
    ("probes", 32, 1280, (1, 64, 256, 5)),
    ("probes", 32, 1282, (1, 64, 256, 6)),
    ("probes", 32, 16384, (1, 64, 256, 64)),
    ("probes", 32, 16386, (1, 64, 256, 65)),
    ("probes", 32, 20482, (1, 64, 256, 81)),
    ("probes", 4096, 16384, (64, 4096, 1024, 16)),
    ("probes", 4096, 16386, (64, 4096, 1280, 13)),
    ("probes", 4096, 20480, (64, 4096, 1280, 16)),
    ("probes", 4096, 20482, (64, 4096, 1536, 14)),
    ("tracers", 37, 1282, (1, 512, 256, 6)),
    ("tracers", 37, 16384, (1, 512, 256, 64)),
    ("tracers", 37, 16386, (1, 512, 512, 33)),
    ("tracers", 37, 20482, (1, 512, 512, 41)),
    ("tracers", 2561, 20482, (6, 3072, 512, 41)),
    ("tracers", 1, 1, (1, 512, 256, 1)),
    ("survey", 20481, 1282, (41, 20992, 256, 6)),
    ("survey", 20481, 16386, (41, 20992, 768, 22)),
    ("survey", 20481, 20480, (41, 20992, 1024, 20)),
    ("survey", 20481, 20482, (41, 20992, 1024, 21)),
    ("survey", 1048576, 1, (2048, 1048576, 256, 1)),
    ("survey_f32", 4097, 20482, (5, 5120, 512, 41)),
    ("tracers_f32x2", 4097, 20482, (5, 5120, 512, 41)),
]
# (point tile, source tile, the ABI's largest count) of every kind
LIMIT = {"probes": "LUDVM_MARCH_MAX_PROBES", "tracers": "LUDVM_MARCH_MAX_TRACERS", "tracers_f32x2": "LUDVM_MARCH_MAX_TRACERS",
         "survey": "LUDVM_MARCH_MAX_SURVEY", "survey_f32": "LUDVM_MARCH_MAX_SURVEY"}
TILES = {"probes": (64, 256), "tracers": (512, 256), "tracers_f32x2": (1024, 256), "survey": (512, 256), "survey_f32": (1024, 256)}
BOUNDS = (0, 1, 255, 256, 257, 16384, 16386, 10 ** 6, 10 ** 7)


def abi_limit(name):
    with open(os.path.join(ROOT, "include", "ludvm_hip.h")) as f:
        return int(re.search(rf"#define {name} (\d+)", f.read()).group(1))


def test_the_kinds_are_the_five_observers():
    assert sorted(plan_rule.OBSERVER_KINDS) == sorted(TILES)


@pytest.mark.parametrize("kind, count, ns_ub, expected", TABLE)
def test_plans_have_the_values_of_the_rules_they_replace(kind, count, ns_ub, expected):
    p = plan_rule.observer_plan(kind, count, ns_ub)
    assert (p.tiles, p.pad, p.chunk, p.nsplit) == expected


@pytest.mark.parametrize("kind", sorted(TILES))
def test_no_step_outruns_the_slab(kind):
    tile, src = TILES[kind]
    counts = sorted({1, tile - 1, tile, tile + 1, 4096, abi_limit(LIMIT[kind])})
    plans = plan_rule.observer_plan(kind, counts, BOUNDS)
    assert len(plans) == len(counts) * len(BOUNDS)
    for (count, ns_ub), p in zip(((c, n) for c in counts for n in BOUNDS), plans):
        where = f"{kind} count={count} ns_ub={ns_ub}: {p}"
        assert (p.point_tile, p.src_tile) == (tile, src), where
        assert p.tiles == -(-count // tile) and p.pad == p.tiles * tile, where
        assert p.chunk % src == 0, where
        assert p.nsplit * p.chunk >= max(ns_ub, 1), where
        assert 1 <= p.nsplit <= p.want, where
        assert p.nsplit * 2 * p.pad * 8 <= p.slab_bytes, where


def test_slabs_have_the_sizes_of_the_rules_they_replace():
    assert plan_rule.observer_plan("probes", 32, 1).slab_bytes == 1 << 20
    assert plan_rule.observer_plan("survey", 1048576, 1).slab_bytes == 16 << 20
    assert plan_rule.observer_plan("survey_f32", 1048576, 1).slab_bytes == 16 << 20
