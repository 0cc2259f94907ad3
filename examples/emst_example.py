"""Euclidean minimum spanning tree by Boruvka rounds over cross_component_nn.

Every round asks, for each current component, for its shortest edge to a point
outside it (one cross_component_nn call: the masked fused L2-NN on the GPU),
adds those edges and merges the components with the pointer-jumping step of
the sparse MST solver. Components at least halve per round, so a few rounds
reach one component.

    python examples/emst_example.py [--rows 20000] [--dim 16]

Points in general position are assumed (all pairwise distances distinct, as
for random data): equal-length edges would need a total order on the edges.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from raft_amd.neighbors import cross_component_nn
from raft_amd.sparse.solver.mst import merge_components


def emst(x: torch.Tensor):
    """Returns (u, v, squared length) of the m-1 tree edges and the rounds."""
    m = x.shape[0]
    labels = torch.arange(m, device=x.device)
    us, vs, ws = [], [], []
    rounds = 0
    while True:
        src, dst, dist, _ = cross_component_nn(x, labels)
        if src.numel() == 0:
            break
        rounds += 1
        # two components that choose each other name the same edge once
        u, v = torch.minimum(src, dst), torch.maximum(src, dst)
        key, first = torch.unique(u * m + v, return_inverse=True)
        pick = torch.full((key.numel(),), src.numel(), device=x.device)
        pick = pick.scatter_reduce(0, first, torch.arange(src.numel(), device=x.device),
                                   "amin")
        us.append(u[pick])
        vs.append(v[pick])
        ws.append(dist[pick])
        labels = merge_components(labels, labels[src], labels[dst])
    return torch.cat(us), torch.cat(vs), torch.cat(ws), rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000)
    ap.add_argument("--dim", type=int, default=16)
    args = ap.parse_args()

    dev = "cuda" if torch.cuda.is_available() else "cpu"
    torch.manual_seed(0)
    x = torch.randn(args.rows, args.dim, device=dev)
    t0 = time.perf_counter()
    u, v, w, rounds = emst(x)
    if dev == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert u.numel() == args.rows - 1, (u.numel(), args.rows)
    print(f"device={dev} points={args.rows}x{args.dim}: {u.numel()} edges in "
          f"{rounds} rounds, {dt:.3f}s, total length {float(w.sqrt().sum()):.4f}")


if __name__ == "__main__":
    main()
