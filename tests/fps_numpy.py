"""numpy restatement of the farthest-point sampling contract of sn_furthest_point_sample (include/samplenet_hip.h), shared by
tests/test_fps_host.py and tests/test_gpu_fps.py: vectorised over the clouds, one FPS step at a time."""
import numpy as np


def fps_restated(xyz, m):
    """xyz (B,N,3) float32 -> idx (B,m) int32.  idx[:, 0] = 0; each step folds the last pick into the running minima
    (d = (dx*dx + dy*dy) + dz*dz in float32, one rounding per operation; cur = d < cur ? d : cur from +inf) and picks the
    first maximum (np.argmax: ties to the lowest index)."""
    P = np.asarray(xyz, dtype=np.float32)
    B, N, _ = P.shape
    out = np.zeros((B, m), np.int32)
    if B == 0 or m <= 1:
        return out
    X, Y, Z = (np.ascontiguousarray(P[:, :, c]) for c in range(3))
    rows = np.arange(B)
    cur = np.full((B, N), np.inf, np.float32)
    last = np.zeros(B, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(1, m):
            dx = X - X[rows, last][:, None]
            dy = Y - Y[rows, last][:, None]
            dz = Z - Z[rows, last][:, None]
            d = (dx * dx + dy * dy) + dz * dz
            cur = np.where(d < cur, d, cur)
            last = np.argmax(cur, axis=1)
            out[:, j] = last
    return out
