"""CPU checks of the contact clusters' restatement (clusters_ref.py) and of the union-find the hook kernel runs (query_core.h: uf_find /
uf_unite, compiled into tools/clusters_check.cpp behind std::atomic): the two restatements against each other, the answer's invariants and
the coarsening of the partition as the margin grows; the host twin under 16 threads -- plain, and as a stand-alone program built with
-fsanitize=thread -- on random graphs, a shuffled 10^5 chain and a clique; its roots on a scene's own pair rows against the restatement; four
mutants, each caught by its named case; cluster_members; the loader's symbol and the header's declaration."""
import os
import subprocess

import numpy as np
import pytest

import clusters_ref as K
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _spheres(centres, radius):
    s = np.zeros((len(centres), 7), F)
    s[:, :3] = centres
    s[:, 3:6] = 0.5
    s[:, 6] = radius
    return s


def _random_scene(n, seed, dup):
    rng = np.random.default_rng(seed)
    s = _spheres(rng.uniform(-40, 40, (n, 3)), rng.uniform(0.3, 2.5, n))
    s[n - dup:, :3] = s[0, :3]                     # coincident centres
    return s


def _chain(n, seed=None):
    """unit spheres in a line, centres 2 apart: each touches only its neighbours at margin 0.  seed: the rows shuffled"""
    c = np.zeros((n, 3))
    c[:, 0] = 2.0 * np.arange(n)
    s = _spheres(c, 1.0)
    return s if seed is None else s[np.random.default_rng(seed).permutation(n)]


def _cloud(n, seed):
    return _spheres(np.random.default_rng(seed).uniform(0.0, 30.0, (n, 3)), 0.0)


SCENES = {
    "rgbbox": (lambda: O.OracleScene("rgbbox").arrays()["L"], (0.0, 0.5, 2.0)),
    "irreg": (lambda: O.OracleScene("irreg").arrays()["L"], (0.0, 0.5, 2.0)),
    "coincident": (lambda: _random_scene(700, 3, 40), (0.0, 1.0, 4.0)),
    "chain": (lambda: _chain(513, 9), (0.0, 0.5)),
    "cloud": (lambda: _cloud(1500, 4), (0.0, 1.2, 2.0, 3.0)),
}


@pytest.fixture(scope="module", params=list(SCENES), ids=list(SCENES))
def answers(request):
    """(L, [(margin, pairs, the union-find's answer)]), computed once"""
    make, margins = SCENES[request.param]
    L = make()
    return request.param, L, [(m, K.pairs(L, m), K.clusters(L, m)) for m in margins]


def test_the_two_restatements_agree(answers):
    name, L, rows = answers
    for margin, _, want in rows:
        got = K.clusters_by_labels(L, margin)
        for a, b in zip(got[:3], want[:3]):
            assert a.dtype == np.int32 and np.array_equal(a, b), (name, margin)
        assert got[3] == want[3]
    if name == "chain":
        assert rows[0][2][3] == 1 and (rows[0][2][0] == 0).all()
    if name == "coincident":
        assert rows[0][2][2].max() >= 40
    if name == "cloud":
        assert rows[0][2][3] == L.shape[0] and 1 < rows[2][2][3] < L.shape[0] and rows[2][2][2].max() > 20


def test_invariants(answers):
    name, L, rows = answers
    n = L.shape[0]
    ar = np.arange(n, dtype=np.int32)
    for margin, pairs, (root, cluster, size, num) in rows:
        assert np.array_equal(root[root], root) and (root <= ar).all()
        assert np.array_equal(root[pairs[:, 0]], root[pairs[:, 1]])                    # every edge inside one cluster
        roots = np.nonzero(root == ar)[0]
        assert num == roots.size and size[roots].sum() == n
        assert np.array_equal(cluster, np.searchsorted(roots, root).astype(np.int32))  # the rank of the root among the roots
        assert np.array_equal(size, np.bincount(cluster, minlength=num)[cluster])
        lowest = np.full(num, n, np.int64)                                              # the root is its component's smallest index
        np.minimum.at(lowest, cluster, ar)
        assert np.array_equal(lowest, roots)
    for (_, _, fine), (_, _, coarse) in zip(rows, rows[1:]):                           # margins ascend: each partition coarsens the last
        assert K.is_coarsening(fine[0], coarse[0]) and coarse[3] <= fine[3], name
    assert not K.is_coarsening(np.array([0, 0, 2]), np.array([0, 1, 1]))


def _tool(target):
    exe = os.path.join(ROOT, "build", target)
    r = subprocess.run(["make", "-C", ROOT, "build/" + target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_host_twin_under_threads():
    r = subprocess.run([_tool("clusters_check"), "threads", "16"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("differ=0") == 7 and "chain 1e5 shuffled" in r.stdout and "clique" in r.stdout, r.stdout


def test_host_twin_under_the_thread_sanitizer():
    """the same program, stand-alone, built with -fsanitize=thread: the right roots and no report"""
    r = subprocess.run([_tool("tsan/clusters_check"), "threads", "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stderr and "ThreadSanitizer" not in r.stdout, r.stderr
    assert r.stdout.count("differ=0") == 7, r.stdout


@pytest.mark.parametrize("mutant, case", [("linking smaller under larger", "min_root"), ("not retrying a failed CAS", "lost_race"),
                                          ("hooking a non-root", "overwritten_link"), ("halving while flattening", "late_halving")])
def test_mutants_are_caught(mutant, case):
    r = subprocess.run([_tool("clusters_check"), "mutants"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.split()[:2] == ["case", case]]
    real = "uf_root passes" if case == "late_halving" else "uf_unite passes"
    assert len(line) == 1 and real in line[0] and f"mutant '{mutant}' caught" in line[0], r.stdout


def test_host_twin_on_a_scenes_pairs(tmp_path):
    """uf_unite over within_ref's pair rows, four threads, against the restatement"""
    exe = _tool("clusters_check")
    for name, margin in (("irreg", 2.0), ("coincident", 1.0), ("cloud", 2.0)):
        L = SCENES[name][0]()
        edges = np.ascontiguousarray(K.pairs(L, margin), np.int32)
        src, dst = tmp_path / f"{name}_edges.bin", tmp_path / f"{name}_roots.bin"
        edges.tofile(src)
        r = subprocess.run([exe, "edges", str(L.shape[0]), str(src), str(dst), "4"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(np.fromfile(dst, np.int32), K.clusters(L, margin)[0]), name


def test_cluster_members_and_declarations():
    import raytracers_amd as R
    from raytracers_amd import api
    cluster = np.array([2, 0, 1, 0, 2, 2, 1], np.int32)
    off, mem = api.cluster_members(cluster, 4)                     # (cluster 3 is empty)
    assert off.dtype == np.int64 and off.tolist() == [0, 2, 4, 7, 7]
    assert mem.dtype == np.int32 and mem.tolist() == [1, 3, 2, 6, 0, 4, 5]
    L = _cloud(400, 8)
    root, cl, size, num = K.clusters(L, 2.5)
    off, mem = api.cluster_members(cl, num)
    for c in range(num):
        m = mem[off[c]:off[c + 1]]
        assert (np.diff(m) > 0).all() and (cl[m] == c).all() and m[0] == root[m[0]] and m.size == size[m[0]]
    back = np.empty_like(cl)
    back[mem] = np.repeat(np.arange(num, dtype=np.int32), np.diff(off))
    assert np.array_equal(back, cl)
    assert api.cluster_members(np.zeros(0, np.int32), 0)[0].tolist() == [0]
    for bad in (np.array([0, 3]), np.array([-1, 0]), np.zeros((2, 2), np.int32), np.array([0.0, 1.0])):
        with pytest.raises(ValueError):
            api.cluster_members(bad, 2)
    from raytracers_amd import _lib
    assert "rt_contact_clusters" in _lib.RT_SYMBOLS and len(_lib.lib.rt_contact_clusters.argtypes) == 7
    for name in ("contact_clusters", "contact_clusters_into", "cluster_members"):
        assert callable(getattr(R, name)), name
    header = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    assert "int rt_contact_clusters(rt_context *ctx, const rt_prepared *ps, float margin, int32_t *root_dev, int32_t *cluster_dev" in header
    assert '"family=clusters"' in header
