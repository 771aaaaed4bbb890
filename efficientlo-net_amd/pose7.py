"""The float64 algebra of [q | t] rows -- q = (w, x, y, z) a rotation, t a translation, p' = R(q) p + t -- that the trackers, the
world map and the place index share.  Pure torch functions on whatever device their first argument lives (array-likes are taken to
the CPU): device-side operators only, no host synchronisation, so a graph capture records them as they are."""
import torch


def qmul(a, b):
    """Hamilton product of quaternions a (4) or (...,4) and b (...,4), elementwise over the leading dimensions."""
    a0, a1, a2, a3 = a.unbind(-1)
    b0, b1, b2, b3 = b.unbind(-1)
    return torch.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                        a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], -1)


def rotate(q, v):
    """R(q) v for ONE unit quaternion q (4) = (w, u) and v (3) or (n,3): v + 2 w (u x v) + 2 u x (u x v)."""
    u = q[1:].expand_as(v)
    c = torch.linalg.cross(u, v)
    return v + 2.0 * q[0] * c + 2.0 * torch.linalg.cross(u, c)


def compose(world64, pose7):
    """W o T: world64 (7) [q | t] (scan n-1 -> world) and pose7 (7) [q | t] (scan n -> scan n-1) -> (7) float64 (scan n -> world):
    q = q_W (x) q_T, renormalised (both are normalised where they are used); t = R(q_W) t_T + t_W."""
    Wp = torch.as_tensor(world64)
    Wp = Wp.to(torch.float64).reshape(7)
    T = torch.as_tensor(pose7).to(device=Wp.device, dtype=torch.float64).reshape(7)
    qw = Wp[:4] / Wp[:4].norm()
    q = qmul(qw, (T[:4] / T[:4].norm()).reshape(1, 4))[0]
    q = q / q.norm()
    return torch.cat([q, rotate(qw, T[4:]) + Wp[4:]])


def rebase(poses64, T):
    """The held poses after the model's frame moved by T: every row P_j of poses64 (n,7) [q | t] (scan j -> the OLD model frame)
    becomes T^-1 o P_j (scan j -> the NEW frame), where T (7) [q | t] carries the new frame into the old one, p_old = R(q) p_new
    + t -- the pose a fit of (new scan, model) returns.  q_new = conj(q_T) (x) q_j, renormalised; t_new = R(q_T)^T (t_j - t_T)."""
    P = torch.as_tensor(poses64)
    P = P.to(torch.float64).reshape(-1, 7)
    T = torch.as_tensor(T).to(device=P.device, dtype=torch.float64).reshape(7)
    q = T[:4] / T[:4].norm()
    qc = torch.cat([q[:1], -q[1:]])
    qn = qmul(qc, P[:, :4] / P[:, :4].norm(dim=1, keepdim=True))
    qn = qn / qn.norm(dim=1, keepdim=True)
    return torch.cat([qn, rotate(qc, P[:, 4:] - T[4:])], 1)
