"""The planner's arithmetic and argument checks (hsr_env_amd/csrc/plan_logic.h: the HSR_EINVAL conditions, the Irwin-Hall normal, the clamp,
the cost recursion, the rank rule, the indexing and shape of the refit's sums, the refit) are plain C++ that the kernels and a host program
both compile, so a stand-alone program (tests/plan_logic_main.cpp) runs them under AddressSanitizer and UndefinedBehaviorSanitizer here, as
tests/test_normalize_logic_sanitized.py does for the normaliser.  Any report fails the test.  The values the program prints are compared
with tests/plan_ref.py on the same inputs: bit for bit, the refit's sigma to one float32 ulp (its fp64 square root is the one rounding
that is not pinned)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import plan_ref as ref

HERE = Path(__file__).resolve().parent
f32 = np.float32


def word(i):
    return ((np.asarray(i, np.uint64) * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xffffffff)).astype(np.uint32)


def val(i):
    return (word(i) >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)


def planted_costs(K):
    k = np.arange(K)
    c = (np.floor(val(300 + k) * f32(8)).astype(f32) * f32(0.125)).astype(f32)
    c[k % 11 == 5] = np.nan
    inf = k % 7 == 3
    c[inf] = np.where(k[inf] & 1, np.inf, -np.inf)
    return c


def hex32(a):
    return [f"{int(x):08x}" for x in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("plan_logic") / "plan_logic"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "plan_logic_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("ok ") and int(lines[-1].split()[1]) > 100
    return [line.split() for line in lines[:-1]]


def rows(printed, tag):
    return [line[1:] for line in printed if line[0] == tag]


def test_plan_logic_under_asan_ubsan(printed):
    assert sorted({line[0] for line in printed}) == ["act", "cost", "rank", "tree", "z"]


def test_z_and_action_are_the_reference(printed):
    i = np.arange(8)
    z = ref.z_from_words(np.stack([word(4 * i + k) for k in range(4)], axis=-1))
    assert rows(printed, "z")[0] == hex32(z)
    mean = ((val(i) * f32(2)).astype(f32) - f32(1)).astype(f32)
    act = ref.clamp((mean + (val(100 + i) * z).astype(f32)).astype(f32), f32(-0.5), f32(0.75))
    assert rows(printed, "act")[0] == hex32(act)


def test_cost_recursion_is_the_reference(printed):
    c = ref.Costs(1)
    for h in range(6):
        d = ref.dist(np.array([val(200 + h), val(210 + h), val(220 + h)], f32), np.array([0.25, 0.5, 0.75], f32))
        c.step([d], [h == 4], [False], h, 0.5)
    assert rows(printed, "cost")[0] == hex32(c.J) + hex32(c.g) + [str(int(c.alive[0])), str(int(c.reach[0]))]


def test_rank_tree_and_refit_are_the_reference(printed):
    ranks = {int(r[0]): np.array(r[1:], int) for r in rows(printed, "rank")}
    trees = {int(r[0]): r[1:] for r in rows(printed, "tree")}
    assert sorted(ranks) == sorted(trees) == [2, 5, 64, 70, 1024]
    for K in ranks:
        keys, finite = ref.cost_keys(planted_costs(K))
        r = ref.ranks(keys)
        assert np.array_equal(ranks[K], r)
        E = min(max(1, K // 4), int(finite.sum()))
        elite = r < E
        x = (val(500 + np.arange(K)) - f32(0.5)).astype(f32).astype(np.float64)
        s = ref.tree_sum(np.where(elite, x, 0.0))
        m = s / np.float64(E)
        sq = ref.tree_sum(np.where(elite, (x - m) * (x - m), 0.0))
        assert trees[K][:3] == [str(E), f"{int(np.float64(s).view(np.uint64)):016x}", f"{int(np.float64(sq).view(np.uint64)):016x}"]
        # the refit through ref.update: one entry (H = nu = 1) whose sampled actions are x, costs that rank as planted
        mean, sigma, el, best, _, failed = ref.update(np.full((1, 1), 0.1, f32), np.full((1, 1), 0.3, f32), x.astype(f32).reshape(1, 1, K), planted_costs(K),
                                                      max(1, K // 4), 0.7, 0.05, np.array([1.5], f32))
        assert failed == 0 and np.array_equal(el, elite) and best == int(np.flatnonzero(r == 0)[0])
        assert trees[K][3] == hex32(mean)[0]
        assert abs(int(trees[K][4], 16) - int(sigma.view(np.uint32)[0, 0])) <= 1
