"""The K1 backward in closed form, in float64, with the sign-tie allowance of every gradient element (tests/test_k1_bwd_resident.py,
tests/test_attention_peaked_gpu.py, tests/test_attention_cases_host.py).  Runs on whatever device its inputs live on.

The K1 backward kernels evaluate z = W_s x + c in different arithmetic (fp32 FMA chain / exact bf16 triple products), so the sign of a
z within rounding of zero can differ between a kernel and float64; lrelu' jumps by 1 - slope there.  The allowance is what those
(edge, channel) pairs can move each gradient element by - computed from the reference, per element."""
import torch as th

NAMES = ["dW_s", "db_s", "dW_d", "db_d", "dattn", "dW_r", "db_r"]
SLOPE = 0.2


def float64_closed_form(data, deg, chunk=2048, stats=None):
    """The K1 backward of a relation with `deg` in-edges per destination, in float64 from the kernels' own fp32 inputs (the saved
    attention included): g = d_out [out > 0]; de_uk = a_uk (G[k].x_u - T[k]); dz_un = de_uk attn[n] lrelu'(z_un).
    Also, per gradient element, the most the (edge, channel) pairs with z within 2^-18 of the size of its terms can move it when
    an fp32 evaluation of z takes the other side of zero (lrelu' jumps by 1 - slope there): the sign-tie allowance.
    data: x_src [N deg, F], x_dst [N, 2], out / d_out [N, >= H] (relation's columns first), a_save [N deg, 4], prm = the seven
    parameters in the order of NAMES (attn flat [H]), N.  Four heads.  stats: a dict whose "ties" / "pairs" receive the number of
    (edge, channel) pairs counted as ties / looked at."""
    x_src, x_dst, out, d_out, a_save, N = (data[k] for k in ("x_src", "x_dst", "out", "d_out", "a_save", "N"))
    W_s, b_s, W_d, b_d, attn = (t.double() for t in data["prm"][:5])
    H, F = W_s.shape
    D = H // 4
    acc = {nm: th.zeros(t.shape, dtype=th.float64, device=t.device) for nm, t in zip(NAMES, data["prm"])}
    tie = {nm: th.zeros(t.shape, dtype=th.float64, device=t.device) for nm, t in zip(NAMES, data["prm"])}
    Wk = W_s.view(4, D, F)
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        n = e - s
        x = x_src[s * deg:e * deg].double().view(n, deg, F)
        a = a_save[s * deg:e * deg].double().view(n, deg, 4)
        xv = x_dst[s:e].double()
        g = d_out[s:e, :H].double() * (out[s:e, :H] > 0)
        G = th.einsum("nkd,kdf->nkf", g.view(n, 4, D), Wk)
        dot = th.einsum("nuf,nkf->nuk", x, G)
        de = a * (dot - (a * dot).sum(1, keepdim=True))
        c = xv @ W_d.T + b_d + b_s
        z = th.einsum("nuf,hf->nuh", x, W_s) + c[:, None, :]
        pos = z > 0
        de_h = de.repeat_interleave(D, dim=2)
        acc["dattn"] += (de_h * th.where(pos, z, SLOPE * z)).sum((0, 1))
        dz = de_h * attn * th.where(pos, 1.0, SLOPE)
        near = z.abs() <= 2.0 ** -18 * (th.einsum("nuf,hf->nuh", x.abs(), W_s.abs()) + c.abs()[:, None, :])
        if stats is not None:
            stats["ties"] = stats.get("ties", 0) + int(near.sum())
            stats["pairs"] = stats.get("pairs", 0) + near.numel()
        jump = (de_h * attn).abs() * (1 - SLOPE) * near
        tie["dattn"] += (de_h.abs() * z.abs() * (1 - SLOPE) * near).sum((0, 1))
        tie["dW_s"] += th.einsum("nuh,nuf->hf", jump, x.abs())
        js = jump.sum(1)
        tie["db_s"] += js.sum(0)
        tie["db_d"] += js.sum(0)
        tie["dW_d"] += js.T @ xv.abs()
        del z, pos, de_h, near, jump
        Sb = th.einsum("nuk,nuf->nkf", a, x).repeat_interleave(D, dim=1)
        acc["dW_s"] += th.einsum("nuh,nuf->hf", dz, x) + th.einsum("nh,nhf->hf", g, Sb)
        dzs = dz.sum(1)
        del dz
        acc["db_s"] += g.sum(0) + dzs.sum(0)
        acc["db_d"] += dzs.sum(0)
        acc["dW_d"] += dzs.T @ xv
        acc["dW_r"] += g.T @ xv
        acc["db_r"] += g.sum(0)
    return [acc[nm] for nm in NAMES], [tie[nm] for nm in NAMES]


def float64_closed_form_ragged(data, off, stats=None):
    """``float64_closed_form`` for a relation whose destinations have the in-degrees of the segment offsets `off` [N + 1]: the
    destinations of every degree are gathered and handed to it as one relation of that constant degree; the sums over the classes are
    the gradients and allowances of the whole relation.  A destination without in-edges reaches W_r / b_r only."""
    off = off.long().cpu()
    deg = off[1:] - off[:-1]
    H = data["prm"][0].shape[0]
    dev = data["x_src"].device
    acc = [th.zeros(t.shape, dtype=th.float64, device=dev) for t in data["prm"]]
    tie = [th.zeros(t.shape, dtype=th.float64, device=dev) for t in data["prm"]]
    for d in th.unique(deg).tolist():
        rows = th.nonzero(deg == d).flatten()
        sub = dict(x_dst=data["x_dst"][rows.to(dev)], out=data["out"][rows.to(dev)][:, :H], d_out=data["d_out"][rows.to(dev)][:, :H],
                   prm=data["prm"], N=int(rows.numel()))
        if d == 0:
            g = sub["d_out"].double() * (sub["out"] > 0)
            acc[5] += g.T @ sub["x_dst"].double()
            acc[6] += g.sum(0)
            continue
        edges = (off[rows].view(-1, 1) + th.arange(d).view(1, -1)).flatten().to(dev)
        sub["x_src"], sub["a_save"] = data["x_src"][edges], data["a_save"][edges]
        r, t = float64_closed_form(sub, d, chunk=max(1, 2048 * 80 // d), stats=stats)
        for i in range(7):
            acc[i] += r[i]
            tie[i] += t[i]
    return acc, tie
