"""Wall time of one scene change on the device, three ways, for rgbbox, irreg, 10^5 and 10^6 random spheres:

  update    Prepared.update_spheres(t)                       rt_prepared_update_spheres: rebuild in place
  prepare   prepare_scene_from_spheres(ctx, t, ...) + free   rt_prepare_scene_device: a new prepared scene from device spheres
  host      t.cpu(), ctx.scene_from_spheres, prepare_scene, free both   the route before the device entries

`t` is a float32 (n, 7) torch tensor on the context's device; the context shares torch's stream.  The three paths take turns (`warmup`
rounds, then `reps` measured ones), so that clock ramps and caches fall on all of them alike; the line reports the median and the minimum
in ms.  Every entry returns after its build has completed, so the host clock brackets the whole change.

usage: python tools/scene_update_probe.py [reps] [warmup]     (one JSON line per scene and path, then a table on stderr)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def oracle_scene(name):
    import oracle_lib as O
    orc = O.OracleScene(name)
    sc = orc.scene
    s = np.ctypeslib.as_array(C.cast(sc.spheres, C.POINTER(C.c_float)), shape=(orc.n * 7,)).reshape(orc.n, 7).copy()
    return s, ((sc.look_from.x, sc.look_from.y, sc.look_from.z), (sc.look_at.x, sc.look_at.y, sc.look_at.z), float(sc.fov))


def random_scene(n, seed=1):
    rng = np.random.default_rng(seed)
    ext = 10.0 * float(n) ** (1.0 / 3.0)
    s = np.zeros((n, 7), np.float32)
    s[:, 0:3] = rng.uniform(-ext, ext, (n, 3))
    s[:, 3:6] = rng.uniform(0.1, 1.0, (n, 3))
    s[:, 6] = rng.uniform(0.3, 2.0, n)
    return s, ((0.0, 0.5 * ext, 3.0 * ext), (0.0, 0.0, 0.0), 50.0)


def timed(paths, reps, warmup):
    """{name: (median ms, min ms)} of the callables in `paths`, run in turns"""
    ts = {name: [] for name, _ in paths}
    for r in range(warmup + reps):
        for name, fn in paths:
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (float(np.median(v)), float(np.min(v))) for name, v in ts.items()}


def main():
    import torch
    import raytracers_amd as R
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    torch.cuda.set_device(0)
    ctx = R.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    h = w = 1000
    rows = []
    for name in ("rgbbox", "irreg", "1e5", "1e6"):
        s, view = oracle_scene(name) if name in ("rgbbox", "irreg") else random_scene(int(float(name)))
        t = torch.from_numpy(s).cuda()
        ps = R.prepare_scene_from_spheres(ctx, t, h, w, *view)
        R.render(h, w, ps)   # (a view with state to reset: the update path pays for that as a caller would)

        def update():
            ps.update_spheres(t)

        def prepare():
            R.prepare_scene_from_spheres(ctx, t, h, w, *view).free()

        def host():
            a = t.cpu().numpy()
            sc = ctx.scene_from_spheres(a, *view)
            R.prepare_scene(h, w, sc).free()
            sc.free()

        res = timed((("update", update), ("prepare", prepare), ("host", host)), reps if len(s) < 500000 else max(5, reps // 4), warmup)
        for path in ("update", "prepare", "host"):
            med, mn = res[path]
            line = {"scene": name, "spheres": len(s), "height": ps.height, "path": path, "median_ms": round(med, 4), "min_ms": round(mn, 4)}
            rows.append(line)
            print(json.dumps(line), flush=True)
        ps.free()
    ctx.close()
    print(f"{'scene':>8} {'spheres':>8} {'update':>9} {'prepare':>9} {'host':>9}   (median ms)", file=sys.stderr)
    for name in ("rgbbox", "irreg", "1e5", "1e6"):
        r = {x["path"]: x for x in rows if x["scene"] == name}
        print(f"{name:>8} {r['update']['spheres']:>8} {r['update']['median_ms']:>9.3f} {r['prepare']['median_ms']:>9.3f} {r['host']['median_ms']:>9.3f}",
              file=sys.stderr)


if __name__ == "__main__":
    main()
