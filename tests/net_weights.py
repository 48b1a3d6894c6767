"""Weight generator of the DDPG forward tests (numpy only): shared by tests/test_gpu_ddpg_stats.py and the modules that import
it from there, and by tests/forward_cases.py, which must stay importable without torch."""
import numpy as np


def make_net(rng, in1, h1, in2_extra, h2, out, ln, w3_scale, b3):
    glorot = lambda i, o: rng.uniform(-1, 1, size=(i, o)) * np.sqrt(6.0 / (i + o))
    w = dict(W1=glorot(in1, h1), b1=0.1 * rng.normal(size=h1), W2=glorot(h1 + in2_extra, h2), b2=0.1 * rng.normal(size=h2),
             W3=rng.uniform(-w3_scale, w3_scale, size=(h2, out)), b3=b3 + 0.05 * rng.normal(size=out))
    if ln:
        w.update(ln1_g=1 + 0.2 * rng.normal(size=h1), ln1_b=0.1 * rng.normal(size=h1),
                 ln2_g=1 + 0.2 * rng.normal(size=h2), ln2_b=0.1 * rng.normal(size=h2))
    return {k: v.astype(np.float32) for k, v in w.items()}


def oracle_kw(w):
    kw = {k: w[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")}
    kw["layer_norm"] = ((w["ln1_g"], w["ln1_b"]), (w["ln2_g"], w["ln2_b"])) if "ln1_g" in w else None
    return kw
