"""Two graph loops over the semiring products (api.spmm_sr / api.spmv_sr) on a device matrix.  Each relaxes between two
ping-pong device buffers with z = x, stops on info.changed == 0 -- one integer per step, read with the call's own
read-back -- and downloads a vector only once, at the end.  The buffers are torch tensors on the config's device."""
import numpy as np

from .api import spmm_sr, spmv_sr


def _device(config):
    import torch
    return torch.device("cuda", config.device) if config is not None else torch.device("cuda")


def sssp(At, sources, config, max_iters=None):
    """Shortest paths from every vertex of `sources`, Bellman-Ford by pull: D <- min(D, At (min,+) D) with spmm_sr, one
    column per source.  ROW i OF THE OPERAND HOLDS THE IN-EDGES OF i: At(i, j) is the weight of the edge j -> i.  For a
    matrix A with A(u, v) the weight of u -> v pass transpose(A).  Weights may be negative.  The loop stops after the
    first step that changes nothing; max_iters (default: At.rows, which a graph without a negative cycle never needs
    more than) bounds it, and converged is False where the last step allowed still changed something -- a negative
    cycle reachable from a source, or a bound set too low.
    Returns (dist, iterations, converged): dist a (rows, len(sources)) float64 numpy array, inf where there is no path;
    iterations the spmm_sr calls made, the one that found nothing to change included."""
    import torch
    n = At.rows
    if At.cols != n:
        raise ValueError(f"sssp: the matrix must be square, not {At.rows} x {At.cols}")
    src = np.asarray(sources, dtype=np.int64).reshape(-1)
    if src.size == 0 or src.min() < 0 or src.max() >= n:
        raise ValueError("sssp: sources must name at least one vertex, each in [0, rows)")
    max_iters = n if max_iters is None else int(max_iters)
    k = int(src.size)
    dev = _device(config)
    cur = torch.full((n, k), float("inf"), dtype=torch.float64, device=dev)
    cur[torch.from_numpy(src).to(dev), torch.arange(k, device=dev)] = 0.0
    nxt = torch.empty_like(cur)
    torch.cuda.current_stream(dev).synchronize()    # (the calls run on the config's stream, torch filled the block on its own)
    iterations, converged = 0, False
    while iterations < max_iters:
        _, info = spmm_sr(At, cur, config, "min_plus", Z=cur, Y=nxt)
        iterations += 1
        cur, nxt = nxt, cur
        if info.changed == 0:
            converged = True
            break
    return cur.cpu().numpy(), iterations, converged


def connected_components(S, config):
    """The connected components of a graph with a SYMMETRIC pattern S (the values are never read): label propagation,
    l <- min(l, S (min,second) l) with spmv_sr from l = 0 .. rows - 1, until a step changes nothing.  The label of a
    vertex is the smallest vertex id of its component.
    Returns (labels, iterations): labels an int64 numpy array of S.rows entries; iterations the spmv_sr calls made, the
    one that found nothing to change included."""
    import torch
    n = S.rows
    if S.cols != n:
        raise ValueError(f"connected_components: the matrix must be square, not {S.rows} x {S.cols}")
    dev = _device(config)
    cur = torch.arange(n, dtype=torch.float64, device=dev)
    nxt = torch.empty_like(cur)
    torch.cuda.current_stream(dev).synchronize()    # (the calls run on the config's stream, torch filled the vector on its own)
    iterations = 0
    while iterations < max(n, 1):
        _, info = spmv_sr(S, cur, config, "min_second", z=cur, y=nxt)
        iterations += 1
        cur, nxt = nxt, cur
        if info.changed == 0:
            break
    return cur.cpu().numpy().astype(np.int64), iterations
