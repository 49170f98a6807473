"""The random scenes of the fuzz campaigns (ray_fuzz.py, query_fuzz.py): both draw a case's scene from the case's seed through here, so a
seed names the same scene in either tool."""
import numpy as np

F = np.float32


def random_scene(rng, max_n):
    """(spheres7 [n, 7] float32, kind): 2 .. max_n spheres (log-uniform) of one of six layouts, at one of four extents"""
    n = int(np.exp(rng.uniform(np.log(2), np.log(max_n))))
    kind = rng.choice(["uniform", "clustered", "grid", "line", "dupes", "shell"])
    s = np.zeros((n, 7), F)
    ext = float(rng.choice([5.0, 40.0, 300.0, 3000.0]))
    if kind == "uniform":
        s[:, 0:3] = rng.uniform(-ext, ext, (n, 3))
    elif kind == "clustered":
        c = rng.uniform(-ext, ext, (max(1, n // 50), 3))
        s[:, 0:3] = c[rng.integers(0, len(c), n)] + rng.normal(0, ext / 40, (n, 3))
    elif kind == "grid":
        k = max(1, int(round(n ** (1 / 3))))
        g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        s[:len(g), 0:3] = (g - k / 2) * (2 * ext / k)
        s[len(g):, 0:3] = rng.uniform(-ext, ext, (n - len(g), 3))
    elif kind == "line":
        s[:, int(rng.integers(0, 3))] = np.linspace(-ext, ext, n)
    elif kind == "dupes":
        base = rng.uniform(-ext, ext, (max(1, n // 7), 3))
        s[:, 0:3] = base[rng.integers(0, len(base), n)]
    else:
        v = rng.normal(0, 1, (n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True) + 1e-9
        s[:, 0:3] = v * ext
    s[:, 3:6] = rng.uniform(0.1, 1.0, (n, 3))
    s[:, 6] = rng.uniform(0.02, 0.2) * ext * rng.uniform(0.2, 1.0, n) if rng.random() < 0.7 else ext * 0.05
    if rng.random() < 0.3:                     # integer centres and radii: exact tangents and ties
        s[:, 0:3] = np.round(s[:, 0:3]); s[:, 6] = np.maximum(np.round(s[:, 6]), 1.0)
    return s.astype(F), kind
