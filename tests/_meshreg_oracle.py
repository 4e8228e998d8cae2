"""Float64 NumPy restatement of the mesh regularisers (ilps_amd/meshreg.py, csrc/meshreg.hip), one mesh at a time, from the
spec's stored fp32 arrays - they are the definition - with the analytic gradient and the magnitudes T the GPU bars use.

    L(v)_i = v_i - sum_k w_ik v_k (0 for a vertex of degree 0),  r = vweight (L(v) - lap_ref)
    E_lap  = 1/V sum_i vweight_i |L(v)_i - lap_ref_i|^2          dE_lap/dv_i  = 2 (r_i [deg_i > 0] - sum_k w_ki r_k) / V
    E_edge = 1/E sum_{i<k, 1/l^2 != 0} q_ik^2, q = |v_i - v_k|^2 / l^2 - 1       dE_edge/dv_i = 4/E sum_k q_ik / l_ik^2 (v_i - v_k)

T of an output = the sum of the magnitudes of everything added up to form it (every product taken with |.| on its
factors, every difference as a sum): what a running error analysis multiplies by the unit roundoff."""
import numpy as np


def brute_one_ring(faces, V):
    """The one-ring as a list of sorted neighbour lists, by walking the faces."""
    nb = [set() for _ in range(V)]
    for f in np.asarray(faces).reshape(-1, 3).tolist():
        for a in f:
            for b in f:
                if a != b:
                    nb[a].add(b)
    return [sorted(s) for s in nb]


def arrays(spec):
    """The spec's arrays in float64 / int64, with the CSR's row of every entry."""
    off = spec.nb_off.astype(np.int64)
    V = len(off) - 1
    deg = np.diff(off)
    w = spec.nb_w.astype(np.float64).reshape(-1, 3)
    return dict(V=V, E=spec.num_edges, off=off, deg=deg, row=np.repeat(np.arange(V), deg), idx=spec.nb_idx.astype(np.int64),
                w=w[:, 0], wt=w[:, 1], il2=w[:, 2],
                lref=np.zeros((V, 3)) if spec.lap_ref is None else spec.lap_ref.astype(np.float64),
                vw=np.ones(V) if spec.vweight is None else spec.vweight.astype(np.float64))


def _scatter(row, vals, V):
    out = np.zeros((V,) + vals.shape[1:])
    np.add.at(out, row, vals)
    return out


def evaluate(verts, spec, g=(1.0, 1.0)):
    """One mesh verts (V, 3) -> dict(terms (2,), T_terms (2,), grad (V, 3) of g . terms, T_grad (V, 3), grad_lap, grad_edge),
    all float64."""
    a = arrays(spec)
    V, E, row, idx = a["V"], a["E"], a["row"], a["idx"]
    v = np.asarray(verts, np.float64).reshape(V, 3)
    has = (a["deg"] > 0)[:, None]
    with np.errstate(all="ignore"):
        s = _scatter(row, a["w"][:, None] * v[idx], V)
        delta = np.where(has, v - s, 0.0) - a["lref"]
        M = np.where(has, np.abs(v) + _scatter(row, np.abs(a["w"])[:, None] * np.abs(v[idx]), V), 0.0) + np.abs(a["lref"])
        r = a["vw"][:, None] * delta
        e_lap = (a["vw"] * (delta * delta).sum(1)).sum() / V
        t_lap = (a["vw"] * (M * M).sum(1)).sum() / V
        d = v[row] - v[idx]
        live = a["il2"] != 0
        q = np.where(live, (d * d).sum(1) * a["il2"] - 1.0, 0.0)
        qm = np.where(live, (d * d).sum(1) * a["il2"] + 1.0, 0.0)
        up = live & (idx > row)
        e_edge = (q[up] ** 2).sum() / E if E > 0 else 0.0
        t_edge = (qm[up] ** 2).sum() / E if E > 0 else 0.0
        g_lap = 2.0 / V * (np.where(has, r, 0.0) - _scatter(row, a["wt"][:, None] * r[idx], V))
        tg_lap = 2.0 / V * (np.where(has, a["vw"][:, None] * M, 0.0)
                            + _scatter(row, np.abs(a["wt"])[:, None] * (a["vw"][:, None] * M)[idx], V))
        if E > 0:
            g_edge = 4.0 / E * _scatter(row, (q * a["il2"])[:, None] * d, V)
            tg_edge = 4.0 / E * _scatter(row, (qm * a["il2"])[:, None] * np.abs(d), V)
        else:
            g_edge, tg_edge = np.zeros((V, 3)), np.zeros((V, 3))
    g0, g1 = float(g[0]), float(g[1])
    return dict(terms=np.array([e_lap, e_edge]), T_terms=np.array([t_lap, t_edge]), grad=g0 * g_lap + g1 * g_edge,
                T_grad=abs(g0) * tg_lap + abs(g1) * tg_edge, grad_lap=g_lap, grad_edge=g_edge)


def adam(D, g, m, v, t, lr, beta1, beta2, eps, mode):
    """One Adam update in float64, the two forms of smplr_fit_step's update 5 with col_scale = gscale = 1 -> D, m, v, t."""
    t1 = t + 1
    m1 = beta1 * m + (1.0 - beta1) * g
    v1 = beta2 * v + (1.0 - beta2) * g * g
    c1, c2 = 1.0 - beta1 ** t1, 1.0 - beta2 ** t1
    with np.errstate(all="ignore"):                       # (0 / 0 where m1 = 0 and eps = 0: not taken below)
        if mode == "keras":
            step = lr * np.sqrt(c2) / c1 * m1 / (np.sqrt(v1) + eps)
        else:
            step = lr / c1 * m1 / (np.sqrt(v1) / np.sqrt(c2) + eps)
    return np.where(m1 != 0, D - step, D), m1, v1, t1


def surface_model():
    """The synthetic model carries no faces and scatters its vertices through the limbs' volume - nothing a scan could be
    sampled from.  This one is a surface: uv_sphere() has SMPL's 6 890 vertices and 13 776 faces; radius 0.5 m, one joint per
    latitude band with the weights blended linearly between neighbouring bands (two non-zeros per row), the synthetic
    model's blend shapes, joint regressor and kinematic tree."""
    import dataclasses
    from ilps_amd.smpl_model import synthetic_smpl_model
    from _render_oracle import uv_sphere
    v, f = uv_sphere()
    V = len(v)
    u = np.clip((1.0 - v[:, 1]) / 2.0 * 24.0 - 0.5, 0.0, 23.0)
    j0 = np.minimum(np.floor(u).astype(np.int64), 22)
    a = (u - j0).astype(np.float32)
    w = np.zeros((V, 24), np.float32)
    w[np.arange(V), j0] = 1.0 - a
    w[np.arange(V), j0 + 1] = a
    m = dataclasses.replace(synthetic_smpl_model(1234), v_template=np.asarray(v, np.float64) * 0.5, weights=w.astype(np.float64),
                            faces=np.asarray(f, np.int32))
    m.validate()
    return m, np.argmax(w, 1)
