"""Cost of the contact clusters (rt_contact_clusters) on one GPU, in the same run as the two things it stands between.  Prints one JSON line per
measurement, in the bracket style of tools/within_probe.py: ms per call from HIP events on a torch stream the context enqueues on, after one
untimed warm-up call; the host route from a wall clock around the whole route, one call per round.

    python tools/clusters_probe.py [--iters N] [--rounds R]

Per case the bracket is measured `rounds` times in turn; the spread of a measurement over the rounds is what a difference between two of them
has to exceed:
  (a) rt_contact_pairs_count alone: the same walk with no unions (and its scan) -- the floor the hook cannot beat;
  (b) the route a caller had before: count + fill (pairs only) + copy to the host + connected components there (scipy's csgraph where it is
      installed, else min-label propagation in numpy; `host` names which);
  (c) rt_contact_clusters with all four outputs; (c') with root alone (init + hook + flatten).
(b)'s roots are compared with (c)'s before anything is timed.

Cases: irreg's self-contacts; the 10^6-sphere floor as prepared, and prepared again from its spheres in shuffled order (the caller's order must
not matter: L is Morton order either way); 1000 and 3000 coincident spheres (a clique: every union contends on one word); 10^6 points of radius 0
with the margin as linking length near the percolation threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracers_amd as R  # noqa: E402

VIEW = ((0.0, 5.0, 40.0), (0.0, 0.0, 0.0), 50.0)

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    HOST = "scipy csgraph"
except ImportError:
    HOST = "numpy min-label"


def host_roots(n, pairs):
    """the smallest index of every component of the (m, 2) edges"""
    if HOST == "scipy csgraph":
        g = coo_matrix((np.ones(pairs.shape[0], np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
        _, label = connected_components(g, directed=False)
        lowest = np.full(label.max() + 1, n, np.int64)
        np.minimum.at(lowest, label, np.arange(n))
        return lowest[label].astype(np.int32)
    e = pairs.astype(np.int64)
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, e[:, 0], label[e[:, 1]])
        np.minimum.at(new, e[:, 1], label[e[:, 0]])
        new = new[new]
        if np.array_equal(new, label):
            return label.astype(np.int32)
        label = new


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def bracket(ctx, ps, margin, iters, rounds, **info):
    n = ps.num_spheres
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    root, cluster, size = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    num = torch.empty(1, dtype=torch.int64, device="cuda")
    count = lambda: R.contact_pairs_count_into(ps, off.data_ptr(), margin)  # noqa: E731
    count()
    total = int(off[n].item())
    pair = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")

    def today():
        count()
        m = int(off[n].item())
        R.contact_pairs_fill_into(ps, off.data_ptr(), m, pair.data_ptr(), None, margin)
        return host_roots(n, pair[:m].cpu().numpy())

    full = lambda: R.contact_clusters_into(ps, root.data_ptr(), cluster.data_ptr(), size.data_ptr(), num.data_ptr(), margin)  # noqa: E731
    only = lambda: R.contact_clusters_into(ps, root.data_ptr(), None, None, None, margin)  # noqa: E731
    want = today()
    full()
    torch.cuda.synchronize()
    assert np.array_equal(root.cpu().numpy(), want), "rt_contact_clusters' roots != the host route's"
    clusters, largest = int(num.item()), int(size.max().item())
    info = dict(info, spheres=n, margin=margin, pairs=total, pair_bytes=8 * total, clusters=clusters, largest=largest)
    for rnd in range(rounds):
        rows = [("(a) contact pairs count + scan", timed(count, iters), "family=within count self")]
        t0 = time.perf_counter()
        today()
        rows.append((f"(b) count + fill + copy + host components ({HOST})", (time.perf_counter() - t0) * 1e3, "host"))
        rows.append(("(c) contact clusters, all outputs", timed(full, iters), ctx.last_launch))
        rows.append(("(c') contact clusters, root only", timed(only, iters), ctx.last_launch))
        for what, ms, launch in rows:
            print(json.dumps(dict(info, what=what, round=rnd, ms=round(ms, 4), launch=launch)), flush=True)


def spheres(centres, radius):
    s = np.zeros((len(centres), 7), np.float32)
    s[:, :3] = centres
    s[:, 3:6] = 0.5
    s[:, 6] = radius
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    for name in ("irreg", "big"):
        scene = ctx.scene(name)
        ps = R.prepare_scene(64, 64, scene)
        bracket(ctx, ps, 0.0, a.iters, a.rounds, case="self-contacts", scene=name, order="as prepared", height=ps.height)
        if name == "big":
            L = ps.bvh_arrays()["L"]
            again = R.prepare_scene_from_spheres(ctx, np.ascontiguousarray(L[rng.permutation(L.shape[0])]), 64, 64, *VIEW)
            bracket(ctx, again, 0.0, a.iters, a.rounds, case="self-contacts", scene=name, order="shuffled input", height=again.height)
            again.free()
        ps.free()
        scene.free()
    for n in (1000, 3000):
        ps = R.prepare_scene_from_spheres(ctx, spheres(np.tile([[1.5, -2.0, 3.25]], (n, 1)), 1.0), 64, 64, *VIEW)
        bracket(ctx, ps, 0.0, a.iters, a.rounds, case="coincident clique", scene=f"clique{n}", order="-", height=ps.height)
        ps.free()
    side = 100.0 * 50.0 ** (1.0 / 3.0)      # the density of the suite's 20 000-point cloud in a cube of side 100
    ps = R.prepare_scene_from_spheres(ctx, spheres(rng.uniform(0.0, side, (1000000, 3)), 0.0), 64, 64, *VIEW)
    bracket(ctx, ps, 3.2, a.iters, a.rounds, case="point cloud, linking length 3.2", scene="cloud1e6", order="-", height=ps.height)
    ps.free()
    ctx.close()


if __name__ == "__main__":
    main()
