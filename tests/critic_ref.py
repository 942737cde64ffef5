"""A float64 numpy restatement of the vocoder critic, written from include/e2etts_critic.h: both discriminator families over a row's own
length, the weight folds of the packer (weight_norm, spectral_norm without a power iteration, the stride fold, the fragment order), the
figures and the order of their reduction, and the bars the GPU tests hold the library to.  No GPU and no torch needed.

``mut`` arguments are the mutations tests/test_critic_host.py shows the bars to catch: "drop_tap" (the last tap of every grouped layer),
"pre_activation" (the map taken before the leaky ReLU), "reflect_repeat" (the edge sample repeated by the reflect extension),
"pool_divisor" (the pool divides by the samples it really covers), "sigma_iter" (sigma after one more power iteration)."""
from __future__ import annotations

import numpy as np

RED_THREADS, RED_PER_LANE = 256, 16
RED_CHUNK = RED_THREADS * RED_PER_LANE


def out_len(n, k, stride, pad):
    v = n + 2 * pad - k
    return 0 if v < 0 else v // stride + 1


def pool_len(n):
    return out_len(n, 4, 2, 2)


def disc_lens(n, layers, period=0, scale=0):
    """[input length, length after each layer (the post layer last)] of a row of n samples."""
    v = -(-n // period) if period else n
    for _ in range(scale):
        v = pool_len(v)
    out = [v]
    for cout, k, s, g, pad in layers:
        v = out_len(v, k, s, pad)
        out.append(v)
    return out


# ---------------------------------------------------------------- weights
def effective_weight(sd, prefix, mut=None):
    """float64 [Cout, Cin / groups, k] of a layer: g v / ||v||, or weight_orig / (u . (W v)) with the stored vectors."""
    if prefix + ".weight_orig" in sd:
        w = np.asarray(sd[prefix + ".weight_orig"], np.float64)
        W = w.reshape(w.shape[0], -1)
        u, v = np.asarray(sd[prefix + ".weight_u"], np.float64), np.asarray(sd[prefix + ".weight_v"], np.float64)
        if mut == "sigma_iter":   # what training mode would do first
            v = W.T @ u
            v /= np.linalg.norm(v)
            u = W @ v
            u /= np.linalg.norm(u)
        out = w / (u @ (W @ v))
    else:
        v = np.asarray(sd[prefix + ".weight_v"], np.float64)
        g = np.asarray(sd[prefix + ".weight_g"], np.float64)
        norm = np.sqrt((v * v).reshape(v.shape[0], -1).sum(1)).reshape(g.shape)
        out = g * v / norm
    return out[..., 0] if out.ndim == 4 else out


def layer_weights(sd, idx, layers, mut=None):
    """[(w [Cout, Cin / groups, k], bias)] of discriminator ``idx`` of a state dict, the post layer last."""
    out = []
    for l in range(len(layers)):
        prefix = f"discriminators.{idx}." + ("conv_post" if l == len(layers) - 1 else f"convs.{l}")
        out.append((effective_weight(sd, prefix, mut), np.asarray(sd[prefix + ".bias"], np.float64)))
    return out


def stride_fold(w, stride, pad):
    """The header's fold: (w' [Cout, K', s * Cin], q)."""
    Cout, Cin, k = w.shape
    q = -(-pad // stride)
    o = stride * q - pad
    kf = -(-(o + k) // stride)
    out = np.zeros((Cout, kf, stride * Cin), w.dtype)
    for jf in range(kf):
        for f in range(stride):
            j = stride * jf + f - o
            if 0 <= j < k:
                out[:, jf, f * Cin:(f + 1) * Cin] = w[:, :, j]
    return out, q


def fold_waste(k, stride, pad):
    """The share of the folded weights that is structural zeros."""
    q = -(-pad // stride)
    kf = -(-(stride * q - pad + k) // stride)
    return 1.0 - k / (kf * stride)


def folded_conv(x, wf, q, stride):
    """The stride-1 convolution of the folded layer on x [T, Cin] viewed as [ceil(T / s), s * Cin] -> [max(out, folded rows), Cout]."""
    T, Cin = x.shape
    Cout, kf, sc = wf.shape
    rows = -(-T // stride)
    xf = np.zeros((rows * stride, Cin), x.dtype)
    xf[:T] = x
    xf = xf.reshape(rows, stride * Cin)
    xp = np.zeros((rows + 2 * kf, sc), x.dtype)
    xp[q:q + rows] = xf
    return sum(xp[j:j + rows] @ wf[:, j, :].T for j in range(kf))


def group_fragments(w, groups):
    """The fragment order of a grouped layer's weights, element by element from the header's index formula."""
    Cout, cin_g, k = w.shape
    cout_g = Cout // groups
    ntp = -(-cout_g // 32)
    out = np.zeros((groups, ntp, k, cin_g // 2, 64), w.dtype)
    for lane in range(64):
        n, half = lane % 32, lane // 32
        for t in range(ntp):
            if t * 32 + n < cout_g:
                rows = np.arange(groups) * cout_g + t * 32 + n
                out[:, t, :, :, lane] = w[rows][:, half::2, :].transpose(0, 2, 1)
    return out.reshape(-1)


# ---------------------------------------------------------------- layers
def conv1d(x, w, b, stride, groups, pad, drop_tap=False):
    """x [T, Cin] -> [out_len(T), Cout] in x's dtype arithmetic (float64 for the reference); zero padding at both ends."""
    T, Cin = x.shape
    Cout, cin_g, k = w.shape
    To = out_len(T, k, stride, pad)
    xp = np.zeros((T + 2 * pad + stride, Cin), x.dtype)
    xp[pad:pad + T] = x
    cout_g = Cout // groups
    y = np.zeros((To, Cout), x.dtype)
    for j in range(k - (1 if drop_tap else 0)):
        xs = xp[j:j + stride * To:stride][:To]
        for g in range(groups):
            y[:, g * cout_g:(g + 1) * cout_g] += xs[:, g * cin_g:(g + 1) * cin_g] @ w[g * cout_g:(g + 1) * cout_g, :, j].T
    return y + b


def lrelu(v, slope):
    return np.where(v >= 0, v, v * slope)


def reflect_fold(x, p, mut=None):
    """[n] -> [ceil(n / p), p]: extended at its end by p - n % p reflected samples (the edge sample is not repeated)."""
    n = x.shape[0]
    if n % p:
        m = p - n % p
        ext = x[n - 2 - np.arange(m)] if mut != "reflect_repeat" else x[n - 1 - np.arange(m)]
        x = np.concatenate([x, ext])
    return x.reshape(-1, p)


def pool(x, mut=None):
    n = x.shape[0]
    xp = np.zeros(n + 6, x.dtype)
    xp[2:2 + n] = x
    To = pool_len(n)
    t = 2 * np.arange(To)
    s = ((xp[t] + xp[t + 1]) + xp[t + 2]) + xp[t + 3]
    if mut == "pool_divisor":
        cnt = sum(((t + i - 2 >= 0) & (t + i - 2 < n)).astype(x.dtype) for i in range(4))
        return s / np.maximum(cnt, 1)
    return s * x.dtype.type(0.25)


def forward_disc(x, weights, layers, slope, period=0, scale=0, mut=None):
    """One row x [n] through one discriminator -> the maps in the reference's layout, [C, T, p] (period) or [C, T] (scale), the post map
    last; its flattened form (t major, column minor) is the score."""
    x = np.asarray(x)
    for _ in range(scale):
        x = pool(x, mut)
    cols = reflect_fold(x, period, mut).T if period else x[None, :]   # [cols, T]
    seqs = [c[:, None] for c in cols]
    maps = []
    for l, ((cout, k, s, g, pad), (w, b)) in enumerate(zip(layers, weights)):
        post = l == len(layers) - 1
        pre = [conv1d(sq, w.astype(x.dtype), b.astype(x.dtype), s, g, pad, drop_tap=(mut == "drop_tap" and g > 1)) for sq in seqs]
        seqs = pre if post else [lrelu(v, x.dtype.type(slope)) for v in pre]
        kept = pre if (mut == "pre_activation" and not post) else seqs
        m = np.stack(kept, axis=-1).transpose(1, 0, 2)   # [C, T, cols]
        maps.append(m if period else m[..., 0])
    return maps


def forward_all(x, cfg, state_mpd, state_msd, mut=None, dtype=np.float64):
    """Every discriminator on one row -> [maps of discriminator 0, ...] (periods first, then scales)."""
    out = []
    x = np.asarray(x, dtype)
    for i, p in enumerate(cfg["periods"]):
        layers = list(cfg["mpd"]) + [cfg["mpd_post"]]
        out.append(forward_disc(x, layer_weights(state_mpd, i, layers, mut), layers, cfg["slope"], period=int(p), mut=mut))
    for i in range(int(cfg["n_scales"])):
        layers = list(cfg["msd"]) + [cfg["msd_post"]]
        out.append(forward_disc(x, layer_weights(state_msd, i, layers, mut), layers, cfg["slope"], scale=i, mut=mut))
    return out


# ---------------------------------------------------------------- figures
def figures(maps_r, maps_g, n_periods):
    """The header's per-row figures from the maps of both sides (plain float64 means)."""
    fm = [[float(np.mean(np.abs(r - g))) for r, g in zip(dr, dg)] for dr, dg in zip(maps_r, maps_g)]
    d_real = [float(np.mean((1.0 - dr[-1]) ** 2)) for dr in maps_r]
    d_fake = [float(np.mean(dg[-1] ** 2)) for dg in maps_g]
    g_fake = [float(np.mean((1.0 - dg[-1]) ** 2)) for dg in maps_g]
    P = n_periods
    return dict(fm=fm, d_real=d_real, d_fake=d_fake, g_fake=g_fake,
                feature_loss_mpd=2.0 * sum(sum(f) for f in fm[:P]), feature_loss_msd=2.0 * sum(sum(f) for f in fm[P:]),
                disc_loss_mpd=sum(a + b for a, b in zip(d_real[:P], d_fake[:P])), disc_loss_msd=sum(a + b for a, b in zip(d_real[P:], d_fake[P:])),
                gen_loss_mpd=sum(g_fake[:P]), gen_loss_msd=sum(g_fake[P:]))


def internal_order(m):
    """A map in the reference's layout ([C, T, p] or [C, T]) flattened in the library's order [column, position, channel]."""
    m = m if m.ndim == 3 else m[..., None]
    return np.ascontiguousarray(m.transpose(2, 1, 0)).reshape(-1)


def _tree(v):
    v = v.copy()
    s = RED_THREADS // 2
    while s >= 1:
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
        s //= 2
    return v[..., 0]


def ordered_sum(vals):
    """The header's reduction of float64 values: lanes of chunks of 4096, a tree over the lanes, the chunks over lanes, the tree again."""
    vals = np.asarray(vals, np.float64).reshape(-1)
    N = vals.size
    nch = -(-max(N, 1) // RED_CHUNK)
    v = np.zeros(nch * RED_CHUNK)
    v[:N] = vals
    v = v.reshape(nch, RED_PER_LANE, RED_THREADS)
    lanes = np.zeros((nch, RED_THREADS))
    for i in range(RED_PER_LANE):
        lanes = lanes + v[:, i, :]
    chunk = _tree(lanes)
    rounds = -(-nch // RED_THREADS)
    c = np.zeros(rounds * RED_THREADS)
    c[:nch] = chunk
    c = c.reshape(rounds, RED_THREADS)
    lane = np.zeros(RED_THREADS)
    for i in range(rounds):
        lane = lane + c[i]
    return float(_tree(lane[None, :])[0])


def ordered_figures(maps_r, maps_g):
    """fm, d_real, d_fake, g_fake from float32 maps in the reference's layout, by the library's reduction, bit for bit."""
    fm = []
    for dr, dg in zip(maps_r, maps_g):
        fm.append([ordered_sum(np.abs(internal_order(r).astype(np.float64) - internal_order(g).astype(np.float64))) / r.size for r, g in zip(dr, dg)])

    def mom(m, one):
        v = internal_order(m).astype(np.float64)
        d = (1.0 - v) if one else v
        return ordered_sum(d * d) / v.size
    return dict(fm=fm, d_real=[mom(d[-1], True) for d in maps_r], d_fake=[mom(d[-1], False) for d in maps_g], g_fake=[mom(d[-1], True) for d in maps_g])


# ---------------------------------------------------------------- bars of a single convolution launch
def conv_case(x, lens, w, b, stride, groups, pad, slope):
    """One launch on x [B, T, Cin] float32 with ragged lens: dict(ref [B, To_cap, Cout] float64 with zeros past a row's own output length,
    S the sum of |terms| per element, n the number of terms, to [B])."""
    B, T, Cin = x.shape
    Cout, cin_g, k = w.shape
    to = [out_len(int(n), k, stride, pad) for n in lens]
    cap = max(max(to), 1)
    ref, S = np.zeros((B, cap, Cout)), np.zeros((B, cap, Cout))
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    for i in range(B):
        xi = x[i, :int(lens[i])].astype(np.float64)
        pre = conv1d(xi, w64, b64, stride, groups, pad)
        ref[i, :to[i]] = lrelu(pre, np.float64(np.float32(slope)))
        S[i, :to[i]] = conv1d(np.abs(xi), np.abs(w64), np.abs(b64), stride, groups, pad)
    return dict(ref=ref, S=S, n=cin_g * k + 2, to=np.asarray(to))


def conv_eval32(x, lens, w, b, stride, groups, pad, slope):
    """The float32 yardstick of tests/kernel_ref.py for this launch, on its FIRST sequence: one rounded product and one rounded addition
    per term in the kernel's order (tap-major, the group's channels ascending within a tap), every group at once -> [To, Cout]."""
    n = int(lens[0])
    Cout, cin_g, k = w.shape
    cout_g = Cout // groups
    To = out_len(n, k, stride, pad)
    xp = np.zeros((n + 2 * pad + stride, x.shape[2]), np.float32)
    xp[pad:pad + n] = x[0, :n]
    wg = w.astype(np.float32).reshape(groups, cout_g, cin_g, k)
    acc = np.zeros((To, groups, cout_g), np.float32)
    for j in range(k):
        xs = xp[j:j + stride * To:stride][:To].reshape(To, groups, cin_g)
        for c in range(cin_g):
            np.add(acc, xs[:, :, c, None] * wg[None, :, :, c, j], out=acc)
    v = acc.reshape(To, Cout) + b.astype(np.float32)
    return np.where(v >= 0, v, v * np.float32(slope)).astype(np.float32)
