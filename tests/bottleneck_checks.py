"""What the GPU tests of the bottleneck distance share (tests/test_gpu_bottleneck.py, tests/test_gpu_bottleneck_classes.py): packing and
solving a batch, one problem's outputs against the restatement of tests/bottleneck_cases.py, and the C entry of csrc/bottleneck.hip called
on a sub-range of a batch into sentinel-filled outputs.  torch is handed in: importing this module needs no GPU."""
import ctypes as C

import numpy as np

import bottleneck_cases as cases


def _pack(torch, problems):
    xoff = np.concatenate([[0], np.cumsum([len(x) for x, _ in problems])]).astype(np.int64)
    yoff = np.concatenate([[0], np.cumsum([len(y) for _, y in problems])]).astype(np.int64)
    X = np.concatenate([x for x, _ in problems] + [np.zeros((0, 2))]).reshape(-1, 2)
    Y = np.concatenate([y for _, y in problems] + [np.zeros((0, 2))]).reshape(-1, 2)
    return xoff, yoff, tuple(torch.as_tensor(a).cuda() for a in (xoff, X, yoff, Y))


def _solve(torch, problems, check=True):
    from tlc_gnn_amd import ops
    xoff, yoff, (dxo, dX, dyo, dY) = _pack(torch, problems)
    r = ops.bottleneck_matching(dxo, dX, dyo, dY, want_grad=True, grad_target=True, check=check)
    h = {k: v.cpu().numpy() for k, v in r.items()}
    for v in h.values():
        v.setflags(write=False)
    return xoff, yoff, h


def _check_witness(X, Y, h, xoff, yoff, b, want):
    """problem b of a solved batch: the value, the matching, the pair it names and the gradients"""
    ax, ay = h["assign_x"][xoff[b]:xoff[b + 1]], h["assign_y"][yoff[b]:yoff[b + 1]]
    dist = h["dist"][b:b + 1]
    print("n=%d m=%d: device %.17g restatement %.17g" % (len(X), len(Y), dist[0], want))
    assert h["status"][b] == 0
    assert np.array_equal(dist.view(np.int64), np.asarray([want], dtype=np.float64).view(np.int64)), (len(X), len(Y), dist[0], want)
    worst = cases.check_matching(X, Y, ax, ay)
    assert worst == dist[0], (len(X), len(Y), worst, dist[0])
    arg = cases.arg_of(X, Y, ax, ay)
    assert tuple(h["arg"][b].tolist()) == arg, (len(X), len(Y), h["arg"][b], arg)
    gx, gy = cases.gradients(X, Y, arg)
    mine_x, mine_y = h["grad"][xoff[b]:xoff[b + 1]], h["grad_target"][yoff[b]:yoff[b + 1]]
    assert np.array_equal(mine_x, gx) and np.array_equal(mine_y, gy)
    # no -0.0 among the zeros
    assert (mine_x[np.signbit(mine_x)] != 0).all() and (mine_y[np.signbit(mine_y)] != 0).all()


def _raw_outputs(torch, B, nx, ny):
    return dict(dist=torch.full((B,), -7.0, dtype=torch.float64, device="cuda"), arg=torch.full((B, 2), -7, dtype=torch.int32, device="cuda"),
                assign_x=torch.full((nx,), -7, dtype=torch.int32, device="cuda"), assign_y=torch.full((ny,), -7, dtype=torch.int32, device="cuda"),
                grad=torch.full((nx, 2), -7.0, dtype=torch.float64, device="cuda"), grad_target=torch.full((ny, 2), -7.0, dtype=torch.float64, device="cuda"),
                status=torch.full((B,), 77, dtype=torch.uint8, device="cuda"))


def _raw_call(o, dxo, dX, dyo, dY, first, count, max_points):
    """the C entry on problems first .. first + count of the packed batch, writing into the batch's own output rows"""
    from tlc_gnn_amd import _lib
    at = lambda t, k: C.c_void_p(t.data_ptr() + k * t.element_size() * (t.shape[1] if t.dim() == 2 else 1))
    rc = _lib.lib().tlc_bottleneck_matching(C.c_int32(count), at(dxo, first), _lib.ptr(dX), at(dyo, first), _lib.ptr(dY), C.c_int32(max_points),
                                            at(o["dist"], first), at(o["arg"], first), _lib.ptr(o["assign_x"]), _lib.ptr(o["assign_y"]),
                                            _lib.ptr(o["grad"]), _lib.ptr(o["grad_target"]), at(o["status"], first), _lib.stream_ptr())
    assert rc == 0, _lib.lib().tlc_last_error()
