"""The Winograd reference pieces the forward's tests share (tests/test_gpu_paths.py, test_gpu_split.py, exact_fusion.py, exact_wino.py):
the 1-D transforms of winograd.hip as matrices, the point numbering of winograd_common.h and the fp64 restatement of what sits between
two Winograd convs (wino_mid.hip).  numpy only; tests/test_forward_checks.py holds mindex to its two earlier spellings and
between_reference to a direct conv2d form."""
import numpy as np

# the 1-D transforms of winograd.hip as matrices: F(4, 3) (points 0, +-1, +-2, inf) and F(3, 3) (points 0, 1, -1, 2, inf); AT is keyed by
# the number of outputs, BT by the number of points
AT = {4: np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64),
      3: np.array([[1, 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 1]], dtype=np.float64)}
BT = {6: np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                   [0, 4, 0, -5, 0, 1]], dtype=np.float64),
      5: np.array([[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]], dtype=np.float64)}

OFFSETS = {"off1": (0, 36, 66, 96), "offA": (0, 25, 45, 65), "offB": (0, 5, 9, 14), "offC": (0, 5, 10, 14)}


def mindex(phases, cy, cx, i, j, offs=OFFSETS):
    """Point numbering of winograd.hip (wino_mindex): class (cy, cx) has NY x NX points."""
    ny, nx, cls = (5 if cy else 6), (5 if cx else 6), 2 * cy + cx
    if phases == 1:
        return offs["off1"][cls] + i * nx + j
    if i < ny - 1 and j < nx - 1:
        return offs["offA"][cls] + i * (nx - 1) + j
    if i == ny - 1 and j < nx - 1:
        return 81 + offs["offB"][cls] + j
    if j == nx - 1 and i < ny - 1:
        return 99 + offs["offC"][cls] + i
    return 117 + cls


def between_reference(M, bias, phases, w1, b1):
    """fp64 restatement: x = relu(A^T M A + bias) per class -> [n, 7, 7, Cin]; t = relu(x W1^T + b1); V = B^T t B per class."""
    _pts, n, cin = M.shape
    x = np.zeros((n, 7, 7, cin))
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = (5 if cy else 6), (5 if cx else 6)
            m = np.stack([np.stack([M[mindex(phases, cy, cx, i, j)] for j in range(nx)], 0) for i in range(ny)], 0)   # [ny, nx, n, c]
            y = np.einsum("oi,ijnc,pj->opnc", AT[3 if cy else 4], m, AT[3 if cx else 4])
            oy, ox = (4 if cy else 0), (4 if cx else 0)
            x[:, oy:oy + y.shape[0], ox:ox + y.shape[1]] = np.transpose(y, (2, 0, 1, 3))
    x = np.maximum(x + bias, 0.0)
    t = np.maximum(x @ w1.T + b1, 0.0) if w1 is not None else x
    cm = t.shape[-1]
    tp = np.zeros((n, 9, 9, cm))
    tp[:, 1:8, 1:8] = t                                     # zero padding 1
    V = np.zeros((121, n, cm))
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = (5 if cy else 6), (5 if cx else 6)
            oy, ox = (4 if cy else 0), (4 if cx else 0)
            d = tp[:, oy:oy + ny, ox:ox + nx]                # window rows oy - 1 .. (padded index = image index + 1)
            v = np.einsum("pi,nijc,qj->pqnc", BT[ny], d, BT[nx])
            for i in range(ny):
                for j in range(nx):
                    V[mindex(1, cy, cx, i, j)] = v[i, j]
    return x, V
