"""numpy restatements of the reference's two display kernels, written from its text (particlebot_kernel_impl.cuh):
updateCol_k (:401-443, with rgbToHsl / hslToRgb / hue2rgb, :351-398) and the calcCOG / calcCOG1 tree (:295-349, driven
by particlebot_cuda.cu:241-281).  Every float32 / float64 cast is where C's usual arithmetic conversions put one."""
import numpy as np

f32, f64 = np.float32, np.float64


def _hue2rgb(p, q, t):
    if t < 0:
        t = f32(t + f32(1))
    if t > 1:
        t = f32(t - f32(1))
    if f64(t) < 1.0 / 6.0:
        return f32(f64(p) + f64(f32(q - p)) * 6.0 * f64(t))
    if f64(t) < 1.0 / 2.0:
        return q
    if f64(t) < 2.0 / 3.0:
        return f32(f64(p) + f64(f32(q - p)) * (2.0 / 3.0 - f64(t)) * 6.0)
    return p


def _hsl_to_rgb(h, s, l):
    if s == 0:
        return l, l, l
    q = f32(f64(l) * (1.0 + f64(s))) if f64(l) < 0.5 else f32(f32(l + s) - f32(l * s))
    p = f32(2.0 * f64(l) - f64(q))
    return (_hue2rgb(p, q, f32(f64(h) + 1.0 / 3.0)), _hue2rgb(p, q, h), _hue2rgb(p, q, f32(f64(h) - 1.0 / 3.0)))


def _rgb_to_hsl(r, g, b):
    mx = max(max(r, g), b)
    mn = min(min(r, g), b)
    l = f32(f32(mx + mn) / f32(2))
    if mx == mn:
        return f32(0), f32(0), l
    d = f32(mx - mn)
    s = f32(f64(d) / (2.0 - f64(mx) - f64(mn))) if f64(l) > 0.5 else f32(d / f32(mx + mn))
    if mx == r:
        h = f32(f64(f32(f32(g - b) / d)) + (6.0 if g < b else 0.0))
    elif mx == g:
        h = f32(f64(f32(f32(b - r) / d)) + 2.0)
    else:
        h = f32(f64(f32(f32(r - g) / d)) + 4.0)
    h = f32(f64(h) / 6.0)
    return h, s, l


def bot_colour(rad, dead, shadowed, min_radius, max_radius, display_shadow, alpha=f32(1)):
    """One bot's RGBA as updateCol_k leaves it (alpha passed through)."""
    rad, mn, mx = f32(rad), f32(min_radius), f32(max_radius)
    if dead:
        return np.array([0, 0, 0, alpha], np.float32)
    a, s = f32(mx - rad), f32(mx - mn)
    r = f32(f32(30) / f32(255))
    with np.errstate(invalid="ignore"):
        g = f32(f32(f32(20) + f32(f32(f32(180) * f32(a * a)) / f32(s * s))) / f32(255))
        b = f32(f32(f32(30) + f32(f32(f32(180) * np.sqrt(f32(rad - mn))) / np.sqrt(s))) / f32(255))
    if display_shadow and shadowed:
        h, sat, l = _rgb_to_hsl(r, g, b)
        r, g, b = _hsl_to_rgb(h, sat, f32(f64(l) / 2.0))
    return np.array([r, g, b, alpha], np.float32)


def colours(rad, dead, shadowed, min_radius, max_radius, display_shadow, alpha=None):
    n = len(rad)
    alpha = np.ones(n, np.float32) if alpha is None else np.asarray(alpha, np.float32)
    return np.array([bot_colour(rad[i], dead[i], shadowed[i], min_radius, max_radius, display_shadow, alpha[i])
                     for i in range(n)], np.float32).reshape(n, 4)


def centroid(pos):
    """calcCOG's value for positions (n, 2) float32: blocks of 64, lane t from 0.0f + v[64b + t] (0.0f past the end),
    s[t] += s[t + k] for k = 32 ... 1, levels until one block remains, then times 1.0f / n and y + 2000.0f."""
    v = np.ascontiguousarray(pos, np.float32).reshape(-1, 2)
    n = v.shape[0]
    mul = f32(f32(1) / f32(n))
    while True:
        m = v.shape[0]
        blocks = (m + 63) // 64
        s = np.zeros((blocks * 64, 2), np.float32)
        s[:m] = np.float32(0) + v  # the add turns -0.0f into +0.0f
        s = s.reshape(blocks, 64, 2)
        k = 32
        while k >= 1:
            s[:, :k] = s[:, :k] + s[:, k:2 * k]
            k //= 2
        v = s[:, 0].copy()
        if blocks == 1:
            break
    out = (v[0] * mul).astype(np.float32)
    out[1] = f32(out[1] + f32(2000))
    return out


def ring_slot(time, interval, steps):
    """ind = (int)(time / hist_int) % hist_steps (C truncation and remainder)."""
    q = f32(f32(time) / f32(interval))
    i = int(q)  # truncation toward zero, as (int)
    return int(np.fmod(i, steps))
