"""Frame state (d3ga_amd/frame_state.py) against the torch lines it replaces, on the GPU: the reference's Embedding forward
(`idxs.max()` on the host, `nn.Embedding(max_norm)`; models/embeddings.py:31-36), its backward, `weight.mean(0, keepdims=True)`
and the pick of one nn.Parameter out of three nn.ParameterDict by a host key (models/garment_net.py:216-222).  Device events
around every call, the two sides alternating call by call in one process: median / p10 / p90 in microseconds at 2 000 and
20 000 frames (32 code dimensions, 87 pose parameters).

    python tools/time_frame_state.py [--iters 200] [--warmup 30] [--out DIR]     -> DIR/frame_state_timing.json (default profiles/)

The events time the op as a user calls it (launches plus the Python layer's enqueue work).  `in_graph` times the HIP ops again
inside a captured graph of 20 calls, one twentieth of a replay: what a call costs a replayed training step.  The torch sides
have no such figure for the lookup and the pick: the one synchronises on `idxs.max()`, the other picks a Python object, and
neither can follow a device index inside a graph -- which is why the HIP ops exist; no speed-up is claimed from these numbers."""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_calib import alternate, fwd_bwd, graph_time, nograd, stats  # noqa: E402  (tools/ is the script's directory)

FRAMES = [2_000, 20_000]
N_DIMS, POSE_WIDTH = 32, 87


def sides(n):
    from d3ga_amd.frame_state import Embedding, FramePoses
    torch.manual_seed(n)
    emb = Embedding(n, N_DIMS).cuda()
    ref = nn.Embedding(n, N_DIMS, max_norm=float(N_DIMS)).cuda()
    with torch.no_grad():
        ref.weight.copy_(emb.frame_embs.weight)
    frame = 7
    cell = torch.tensor([frame], dtype=torch.int32, device="cuda")
    up = torch.randn(1, N_DIMS, 1, 1, device="cuda")

    def aten_fwd():                                          # models/garment_net.py:168-171 with models/embeddings.py:31-36
        idxs = torch.tensor([frame]).cuda()
        if idxs.max() >= n:
            idxs = idxs.clamp(max=n - 1)
        return ref(idxs).reshape(1, N_DIMS, 1, 1)
    hip_fwd = lambda: emb(cell)
    with torch.no_grad():
        assert torch.equal(hip_fwd(), aten_fwd())

    def hip_avg():
        emb._avg = (None, None)                              # (time the computation, not the cache)
        return emb.average()
    aten_avg = lambda: ref.weight.mean(0, keepdims=True)

    g = np.random.default_rng(n)
    smplx = {"seq": {i: {"Rh": g.normal(size=3).astype(np.float32), "Th": g.normal(size=3).astype(np.float32),
                         "poses": g.normal(size=POSE_WIDTH).astype(np.float32)} for i in range(n)}}
    fp = FramePoses(smplx).cuda()
    dicts = [nn.ParameterDict({k: nn.Parameter(c.table[i:i + 1].clone()) for i, k in enumerate(fp.keys)}) for c in fp.caches]
    from d3ga_amd.optim import ClipAdam
    fp.attach(ClipAdam(fp.get_parameters(), lr=1e-3, max_norm=2.5))
    cells = [torch.tensor([i], dtype=torch.int32, device="cuda") for i in (3, n - 1)]
    turn = [0]

    def hip_select():                                        # 12 pairs, a different row every call: write-back + stage
        turn[0] ^= 1
        fp.select(cells[turn[0]])

    def dict_pick():                                         # the reference: a host string key, three dictionary lookups
        k = f"seq_{str(3 + turn[0]).zfill(5)}"
        return dicts[0][k], dicts[1][k], dicts[2][k]

    timed = {"lookup_fwd": {"hip": nograd(hip_fwd), "aten": nograd(aten_fwd)},
             "lookup_fwd_bwd": {"hip": fwd_bwd(hip_fwd, (emb.frame_embs.weight,), up), "aten": fwd_bwd(aten_fwd, (ref.weight,), up)},
             "average": {"hip": hip_avg, "aten": nograd(aten_avg)},
             "select": {"hip": hip_select, "aten": dict_pick}}
    graphed = {"lookup_fwd": nograd(hip_fwd), "lookup_fwd_bwd": fwd_bwd(hip_fwd, (emb.frame_embs.weight,), up), "select": hip_select}
    return timed, graphed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    os.makedirs(a.out, exist_ok=True)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "n_dims": N_DIMS, "pose_width": POSE_WIDTH,
           "frames": {}}
    for n in FRAMES:
        timed, graphed = sides(n)
        r = {}
        for what, fns in timed.items():
            us = alternate(fns, max(a.iters, 100), max(a.warmup, 20))
            r[what] = {k: stats(v) for k, v in us.items()}
            print(f"N={n} {what}: hip {r[what]['hip']} aten {r[what]['aten']}")
        r["in_graph_us"] = {what: round(graph_time(fn), 2) for what, fn in graphed.items()}
        print(f"N={n} in a replayed graph, us per call: {r['in_graph_us']}")
        rec["frames"][str(n)] = r
    json.dump(rec, open(os.path.join(a.out, "frame_state_timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
