"""The triangle renderer (csrc/render.hip, ilps_amd.render) restated in NumPy, and the meshes its tests draw.

* `sample_space`  the vertex stage's mapping in float32, operation for operation (the kernel is built with FMA
                  contraction off): fixed-point x, y with 8 sub-pixel bits, the depth term q, the validity bit.
* `raster`        exact int64 edge functions and the top-left rule; the depth key in float32 exactly as the kernel forms
                  it, so the face map compares bit for bit; returns the face map and, optionally, per-sample coverage
                  counts (the partition property).
* `shade`         depth and colour of a face map in float64 from the exact barycentrics.
* `lambert_colors`, `part_colors`  per-vertex colours in float64.
Generated meshes: `uv_sphere` (84 x 82: SMPL's V = 6 890 and F = 13 776), `soup`, `slivers`, `grid_plane`.
"""
import numpy as np

f32 = np.float32
GUARD = 32768.0
NO_KEY = np.iinfo(np.uint64).max


def sample_space(verts, cam, mode, H, scale=1.0, trans=None, near=0.0, far=1e30):
    """One mesh (V, 3) -> xi, yi (int64 fixed point), q (float32), ok (bool), as mesh_vertex_kernel computes them."""
    v = np.asarray(verts, np.float32)
    X, Y, Z = v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()
    with np.errstate(all="ignore"):
        if trans is not None:
            t = np.asarray(trans, np.float32)
            X, Y, Z = X + t[0], Y + t[1], Z + t[2]
        s = f32(scale)
        c = np.asarray(cam, np.float32)
        if mode == "ortho":
            sx = s * (c[2] + c[0] * X)
            sy = f32(H - 1) - s * (c[3] + c[1] * Y)
            q = Z
            ok = np.ones(len(v), bool)
        else:
            sx = s * ((c[0] * X) / Z + c[1])
            sy = s * ((c[0] * Y) / Z + c[2])
            q = f32(1.0) / Z
            ok = (Z > max(f32(near), f32(0))) & (Z <= f32(far))
        ok &= np.isfinite(sx) & np.isfinite(sy) & np.isfinite(q) & (np.abs(sx) <= GUARD) & (np.abs(sy) <= GUARD)
        xi = np.where(ok, np.rint(sx * f32(256)), 0).astype(np.int64)
        yi = np.where(ok, np.rint(sy * f32(256)), 0).astype(np.int64)
    return xi, yi, q.astype(np.float32), ok


def _edge(ax, ay, bx, by, sx, sy):
    return (bx - ax) * (sy - ay) - (by - ay) * (sx - ax)


def _bias(dx, dy):
    return np.where((dy > 0) | ((dy == 0) & (dx < 0)), 0, 1)


def _ordered(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def _setup(xi, yi, q, ok, faces, H, W):
    """Faces that can cover a sample: indices in range, valid vertices, non-zero area, a bounding box on the image;
    oriented to positive area.  Returns a dict of per-face arrays."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(xi)
    fid = np.arange(len(f))
    good = np.all((f >= 0) & (f < V), axis=1)
    f, fid = f[good], fid[good]
    good = ok[f].all(axis=1)
    f, fid = f[good], fid[good]
    x, y = xi[f], yi[f]
    j0 = np.maximum((x.min(1) + 255) >> 8, 0)
    j1 = np.minimum(x.max(1) >> 8, W - 1)
    r0 = np.maximum((y.min(1) + 255) >> 8, 0)
    r1 = np.minimum(y.max(1) >> 8, H - 1)
    A = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    good = (j0 <= j1) & (r0 <= r1) & (A != 0)
    f, fid, x, y, A, j0, j1, r0, r1 = f[good], fid[good], x[good], y[good], A[good], j0[good], j1[good], r0[good], r1[good]
    neg = A < 0
    for arr in (f, x, y):
        arr[neg, 1], arr[neg, 2] = arr[neg, 2].copy(), arr[neg, 1].copy()
    A = np.abs(A)
    return dict(f=f, fid=fid, x=x, y=y, A=A, j0=j0, j1=j1, r0=r0, r1=r1, q=q[f])


def _edges_at(s, idx, jj, rr):
    x, y = s["x"][idx], s["y"][idx]
    sx, sy = jj * 256, rr * 256
    e0 = _edge(x[:, 1], y[:, 1], x[:, 2], y[:, 2], sx, sy)
    e1 = _edge(x[:, 2], y[:, 2], x[:, 0], y[:, 0], sx, sy)
    e2 = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], sx, sy)
    return e0, e1, e2


def raster(xi, yi, q, ok, faces, H, W, counts=False, chunk=1 << 22):
    """The face map (H, W) int64 (-1 background) of one mesh, by mesh_raster_kernel's rule; with counts=True also the
    number of faces covering each sample (H, W)."""
    s = _setup(xi, yi, q, ok, faces, H, W)
    best = np.full(H * W, NO_KEY, np.uint64)
    cnt = np.zeros(H * W, np.int64)
    n = (s["j1"] - s["j0"] + 1) * (s["r1"] - s["r0"] + 1)
    x, y = s["x"], s["y"]
    b0 = _bias(x[:, 2] - x[:, 1], y[:, 2] - y[:, 1])
    b1 = _bias(x[:, 0] - x[:, 2], y[:, 0] - y[:, 2])
    b2 = _bias(x[:, 1] - x[:, 0], y[:, 1] - y[:, 0])
    start = 0
    while start < len(n):
        stop = start + max(1, int(np.searchsorted(np.cumsum(n[start:]), chunk)))
        idx = np.repeat(np.arange(start, stop), n[start:stop])
        first = np.repeat(np.cumsum(n[start:stop]) - n[start:stop], n[start:stop])
        local = np.arange(len(idx)) - first
        bw = (s["j1"] - s["j0"] + 1)[idx]
        jj = s["j0"][idx] + local % bw
        rr = s["r0"][idx] + local // bw
        e0, e1, e2 = _edges_at(s, idx, jj, rr)
        inside = (e0 >= b0[idx]) & (e1 >= b1[idx]) & (e2 >= b2[idx])
        idx, jj, rr, e0, e1, e2 = idx[inside], jj[inside], rr[inside], e0[inside], e1[inside], e2[inside]
        pix = rr * W + jj
        if counts:
            np.add.at(cnt, pix, 1)
        qq = s["q"][idx]
        with np.errstate(all="ignore"):
            d = ((e0.astype(np.float32) * qq[:, 0] + e1.astype(np.float32) * qq[:, 1])
                 + e2.astype(np.float32) * qq[:, 2]) / s["A"][idx].astype(np.float32)
            keep = d == d
            key = (_ordered(f32(0) - d[keep]) << np.uint64(32)) | s["fid"][idx][keep].astype(np.uint64)
        np.minimum.at(best, pix[keep], key)
        start = stop
    face = np.where(best == NO_KEY, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64))
    face = face.reshape(H, W)
    return (face, cnt.reshape(H, W)) if counts else face


def shade(face, xi, yi, verts, faces, mode, vcol, trans=None):
    """Depth (H, W) and colour (H, W, 3) in float64 of a face map: exact barycentrics, linear in screen space (ortho)
    or perspective-correct (weights lambda_i / z_i).  Background: depth 0, colour NaN (the caller composites)."""
    H, W = face.shape
    Z = np.asarray(verts, np.float64)[:, 2] + (0.0 if trans is None else float(np.asarray(trans, np.float32)[2]))
    depth = np.zeros((H, W))
    rgb = np.full((H, W, 3), np.nan)
    rr, jj = np.nonzero(face >= 0)
    if rr.size == 0:
        return depth, rgb
    f = np.asarray(faces, np.int64)[face[rr, jj]].copy()
    x, y = xi[f], yi[f]
    A = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    neg = A < 0
    for arr in (f, x, y):
        arr[neg, 1], arr[neg, 2] = arr[neg, 2].copy(), arr[neg, 1].copy()
    s = {"x": x, "y": y}
    e = np.stack(_edges_at(s, np.arange(len(f)), jj, rr), axis=1).astype(np.float64)
    lam = e / e.sum(axis=1, keepdims=True)
    z = Z[f]
    if mode == "ortho":
        w = lam
        depth[rr, jj] = (lam * z).sum(1)
    else:
        w = lam / z
        depth[rr, jj] = 1.0 / w.sum(1)
    w = w / w.sum(1, keepdims=True)
    rgb[rr, jj] = np.einsum("pk,pkc->pc", w, np.asarray(vcol, np.float64)[f])
    return depth, np.clip(rgb, 0, 1)


def vertex_normals(verts, faces):
    """normalise(sum over incident faces of (v1 - v0) x (v2 - v0)), 0 where the sum is zero; faces with a non-finite
    cross product are left out."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    with np.errstate(all="ignore"):
        c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    c[~np.isfinite(c).all(1)] = 0
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], c)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0.0)


def lambert_colors(verts, faces, albedo, lights, trans=None):
    """albedo * sum_k c_k max(0, n . normalise(p_k - v)), clipped to [0, 1] (renderer.py:146-197), float64."""
    n = vertex_normals(verts, faces)
    p = np.asarray(verts, np.float64) + (0.0 if trans is None else np.asarray(trans, np.float32).astype(np.float64))
    acc = np.zeros_like(p)
    for pos, col in lights:
        L = np.asarray(pos, np.float64) - p
        ll = np.linalg.norm(L, axis=1, keepdims=True)
        L = np.where(ll > 0, L / np.where(ll > 0, ll, 1), L)
        with np.errstate(invalid="ignore"):
            acc += np.asarray(col, np.float64) * np.maximum((n * L).sum(1, keepdims=True), 0)
    return np.clip(np.asarray(albedo, np.float64) * acc, 0, 1)


def render(verts, faces, cam, mode, H, W, vcol, scale=1.0, trans=None, near=0.0, far=1e30, face_part=None, bg=None):
    """All five maps of one mesh: face (fp32 key, exact), part, alpha, and depth / rgb in float64."""
    xi, yi, q, ok = sample_space(verts, cam, mode, H, scale, trans, near, far)
    face = raster(xi, yi, q, ok, faces, H, W)
    depth, rgb = shade(face, xi, yi, verts, faces, mode, vcol, trans)
    alpha = face >= 0
    back = np.ones((H, W, 3)) if bg is None else np.asarray(bg, np.float64)
    rgb = np.where(alpha[..., None], rgb, back)
    part = np.zeros((H, W), np.uint8) if face_part is None else np.where(alpha, np.asarray(face_part)[np.maximum(face, 0)], 0)
    return dict(face=face, depth=depth, rgb=rgb, alpha=alpha, part=part.astype(np.uint8))


# ---- generated meshes ----------------------------------------------------------------------------------------------

def uv_sphere(segments=84, rings=82):
    """Unit sphere: `rings` latitude circles of `segments` vertices plus two poles, faces wound outward.  84 x 82 gives
    SMPL's counts, V = 6 890 and F = 13 776."""
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None],
                     np.sin(th)[:, None] * np.sin(ph)[None]], axis=-1).reshape(-1, 3)
    v = np.concatenate([[[0, 1, 0]], ring, [[0, -1, 0]]])
    idx = lambda r, k: 1 + r * segments + (k % segments)
    f = []
    for k in range(segments):
        f.append((0, idx(0, k + 1), idx(0, k)))
        for r in range(rings - 1):
            a, b, c, d = idx(r, k), idx(r, k + 1), idx(r + 1, k), idx(r + 1, k + 1)
            f.append((a, b, c))
            f.append((b, d, c))
        f.append((len(v) - 1, idx(rings - 1, k), idx(rings - 1, k + 1)))
    return v, np.asarray(f, np.int32)


def posed_sphere(seed, B=1, radius=0.8):
    """B placed and posed copies: a random rotation, an ellipsoid stretch and a shift; vertices (B, V, 3) float32."""
    v, f = uv_sphere()
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        qn = rng.normal(size=(3, 3))
        Q, _ = np.linalg.qr(qn)
        st = np.diag(rng.uniform(0.7, 1.1, 3))
        out.append(v @ st @ Q.T * radius + rng.uniform(-0.15, 0.15, 3))
    return np.asarray(out, np.float32), f


def soup(seed, n=300, span=1.0):
    """n random triangles in [-span, span]^3 that interpenetrate; vertices (3 n, 3) float32."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-span, span, (n, 1, 3))
    v = c + rng.normal(0, 0.25 * span, (n, 3, 3))
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def slivers(seed, n=24, span=1.0):
    """Long thin triangles crossing the whole image (many tiles) in every direction, at random depths."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1) * 1.4 * span
    c = rng.uniform(-0.3, 0.3, (n, 3)) * span
    w = np.stack([-np.sin(a), np.cos(a), np.zeros(n)], 1) * rng.uniform(0.002, 0.03, (n, 1)) * span
    z = rng.uniform(-0.5, 0.5, (n, 3))
    v = np.stack([c - d, c + d, c + w], 1)
    v[:, :, 2] = z
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def grid_plane(nx, ny, x0, y0, step, z=0.5, alt=True):
    """A tessellated plane of (nx + 1) x (ny + 1) vertices at (x0 + i step, y0 + j step, z), two triangles per cell
    with alternating diagonals (alt) so that vertices carry fans of 4 and of 8 triangles."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    v = np.stack([x0 + i * step, y0 + j * step, np.full(i.shape, z)], -1).reshape(-1, 3)
    f = []
    for r in range(ny):
        for c in range(nx):
            a, b, d, e = r * (nx + 1) + c, r * (nx + 1) + c + 1, (r + 1) * (nx + 1) + c, (r + 1) * (nx + 1) + c + 1
            if alt and (r + c) % 2:
                f += [(a, b, e), (a, e, d)]
            else:
                f += [(a, b, d), (b, e, d)]
    return v.astype(np.float32), np.asarray(f, np.int32)
