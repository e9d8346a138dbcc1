"""Record the reference's own Embedding (models/embeddings.py:13-36) on the CPU as the fixture of the frame-code kernels:

    python tools/gen_frame_state_golden.py --reference /path/to/D3GA      -> tests/golden/frame_state_cases.npz

Needs only torch and numpy.  Per case c<i>: the table before the forward, the table after it (nn.Embedding(max_norm) renorms the
looked-up rows in place), the output, a recorded upstream gradient with the dense weight gradient it gives, and average() of
the table before.  Cases: D in {1, 5, 32} x N in {1, 7}, every idx with a duplicate and an index >= N (the reference clamps
it), rows on both sides of max_norm = D; and two constructed rows with max_norm = 5: (3,4,0,0,0), whose norm EQUALS max_norm
and must not be scaled, and (6,8,0,0,0), which must be.  The upstream gradient is normal; with N = 1, where all three indices
name the one row and the kernel's three-term float32 sum is compared RELATIVELY, it is positive (no cancellation).  The random
tables are drawn again until no row's norm lies within 1e-3 (relative) of max_norm, so that the decision does not hang on the
order of a float32 sum; asserted below."""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(path):
    spec = importlib.util.spec_from_file_location("ref_embeddings", os.path.join(path, "models", "embeddings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Embedding


def clear_of_the_threshold(table, max_norm):
    norms = np.sqrt((table.astype(np.float64) ** 2).sum(1))
    return bool(np.all(np.abs(norms - max_norm) > 1e-3 * max_norm)), norms


def record(Embedding, n, d, idx, table, seed):
    emb = Embedding(n, d)
    emb.frame_embs.weight.data.copy_(torch.from_numpy(table))
    avg = emb.average().detach().numpy().copy()
    out = emb(torch.tensor(idx, dtype=torch.long))
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed))
    if n == 1:              # every index names row 0: a sum of three terms, held to a RELATIVE bar -- the terms share a sign
        dout = dout.abs() + 0.25
    out.backward(dout)
    return {"n": np.int64(n), "d": np.int64(d), "idx": np.asarray(idx, np.int64), "max_norm": np.float64(emb.frame_embs.max_norm),
            "before": table.copy(), "after": emb.frame_embs.weight.detach().numpy().copy(),
            "out": out.detach().numpy().reshape(len(idx), d).copy(), "dout": dout.numpy().reshape(len(idx), d).copy(),
            "dweight": emb.frame_embs.weight.grad.numpy().copy(), "average": avg}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of facebookresearch/D3GA")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "frame_state_cases.npz"))
    a = ap.parse_args()
    Embedding = load_reference(a.reference)
    cases = []
    for d in (1, 5, 32):
        for n in (1, 7):
            idx = [0, 2, 0] if n == 1 else [3, 9, 3, 0, 5]          # a duplicate, and an index >= N that the reference clamps
            # std: Embedding draws normal(0, std), a row's norm is about std sqrt(D) against max_norm = D.  N = 7: std = sqrt(D)
            # puts rows on both sides; N = 1: D = 5 stays below (std = 0.3 sqrt(D)), D = 1 and 32 go above (2 sqrt(D))
            std = float(np.sqrt(d)) * (1.0 if n > 1 else (0.3 if d == 5 else 2.0))
            seed = 1000 * d + n
            while True:
                torch.manual_seed(seed)
                table = Embedding(n, d, std=std).frame_embs.weight.detach().numpy().copy()
                ok, norms = clear_of_the_threshold(table, float(d))
                looked = norms[np.clip(idx, 0, n - 1)]
                want = (looked > d).any() and (looked < d).any() if n > 1 else ((looked > d).all() if d != 5 else (looked < d).all())
                if ok and want:
                    break
                seed += 7919
            assert clear_of_the_threshold(table, float(d))[0]
            cases.append(record(Embedding, n, d, idx, table, seed))
    table = np.array([[3, 4, 0, 0, 0], [6, 8, 0, 0, 0], [0.25, -0.5, 1, 0, 2]], np.float32)
    cases.append(record(Embedding, 3, 5, [0, 1, 1, 7], table, 5))
    assert np.array_equal(cases[-1]["after"][0], table[0]) and not np.array_equal(cases[-1]["after"][1], table[1])
    flat = {"n_cases": np.int64(len(cases))}
    for i, c in enumerate(cases):
        flat.update({f"c{i}_{k}": v for k, v in c.items()})
    np.savez_compressed(a.out, **flat)
    print(f"{len(cases)} cases -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
