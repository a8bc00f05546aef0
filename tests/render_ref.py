"""numpy restatement of the headless frame (Particlebot::writeFrame) as a per-pixel rule, in float32.

With scale = 0.5f * height / halfExtent, px(x) = 0.5f * width - (x - centerX) * scale and
py(y) = 0.5f * height - (y - centerY) * scale, a disc (x, y, r) covers pixel (xx, yy) iff the pixel lies in the clamped
floorf / ceilf bounding box and dx * dx + dy * dy <= pr * pr with dx = (float)xx + 0.5f - px(x), pr = r * scale.  A pixel
takes the colour of the LAST item of the painter's order that covers it: background 245; rectangle obstacles (110, the
inclusive floorf / ceilf box, x mirrored); circle obstacles (110); the light (250, 210, 40); the bots in original index
order; in the reference style the recorded trail slots as red discs of centroid_radius at (x, y - 2000).

tests/test_render_api.py pins this file to the host writer's bytes on the CPU; the GPU tests then use it where no host
writer exists (Sim / Ensemble states)."""
import numpy as np

f32 = np.float32


def scene_from(p, light_radius=None):
    """The fields a frame reads, from anything that names them like SimParams (FlatConfig, OrcParams, SimParams)."""
    nr, nc = int(p.nobstacles), int(p.n_cir_obstacles)
    s = dict(min_radius=f32(p.min_radius), max_radius=f32(p.max_radius), light_x=f32(p.light_x), light_y=f32(p.light_y),
             centroid_radius=f32(p.centroid_radius),
             rects=[(f32(p.x1obs[k]), f32(p.x2obs[k]), f32(p.y1obs[k]), f32(p.y2obs[k])) for k in range(nr)],
             circles=[(f32(p.x_cir_obs[k]), f32(p.y_cir_obs[k]), f32(p.r_cir_obs[k])) for k in range(nc)])
    s["light_radius"] = f32(p.light_radius if light_radius is None else light_radius)
    return s


class View:
    def __init__(self, width, height, center, half_extent):
        self.w, self.h = int(width), int(height)
        self.cx, self.cy = f32(center[0]), f32(center[1])
        self.scale = f32(f32(f32(0.5) * f32(self.h)) / f32(half_extent))
        self.hw, self.hh = f32(f32(0.5) * f32(self.w)), f32(f32(0.5) * f32(self.h))

    def px(self, x):
        return (self.hw - (np.asarray(x, f32) - self.cx) * self.scale).astype(f32)

    def py(self, y):
        return (self.hh - (np.asarray(y, f32) - self.cy) * self.scale).astype(f32)


def _box(v, c, pr):
    """Clamped inclusive pixel ranges of discs with pixel centres c and pixel radii pr along an axis of v pixels."""
    lo = np.maximum(0, np.floor((c - pr).astype(f32)).astype(np.int64))
    hi = np.minimum(v - 1, np.ceil((c + pr).astype(f32)).astype(np.int64))
    return lo, hi


def _paint_disc(img, V, x, y, r, rgb):
    cx, cy = V.px(x), V.py(y)
    pr = f32(f32(r) * V.scale)
    if not (np.isfinite(cx) and np.isfinite(cy) and np.isfinite(pr)):
        return  # the rule of _paint_many's `ok`: such a disc paints nothing
    (x0, x1), (y0, y1) = _box(V.w, cx, pr), _box(V.h, cy, pr)
    if x0 > x1 or y0 > y1:
        return
    dx = ((np.arange(x0, x1 + 1).astype(f32) + f32(0.5)).astype(f32) - cx).astype(f32)
    dy = ((np.arange(y0, y1 + 1).astype(f32) + f32(0.5)).astype(f32) - cy).astype(f32)
    d2 = ((dx * dx).astype(f32)[None, :] + (dy * dy).astype(f32)[:, None]).astype(f32)
    img[y0:y1 + 1, x0:x1 + 1][d2 <= f32(pr * pr)] = rgb


def plain_colours(rad, dead, min_radius, max_radius):
    """uint8 (n, 3): dead black; else R 30 and the truncated clamped G and B of writeFrame (span > 0 guard included)."""
    rad = np.asarray(rad, f32)
    mn, mx = f32(min_radius), f32(max_radius)
    span = f32(mx - mn)
    if span > 0:
        g = ((mx - rad).astype(f32) / span).astype(f32)
        b = ((rad - mn).astype(f32) / span).astype(f32)
    else:
        g = b = np.zeros_like(rad)
    G = (f32(20) + ((f32(180) * g).astype(f32) * g).astype(f32)).astype(f32)
    B = (f32(30) + (f32(180) * np.sqrt(np.where(b > 0, b, f32(0)).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    clamp = lambda v: np.where(v < f32(255), np.where(v > 0, v, f32(0)), f32(255)).astype(f32).astype(np.uint8)
    out = np.stack([np.full(rad.shape, 30, np.uint8), clamp(G), clamp(B)], axis=1)
    out[np.asarray(dead) != 0] = 0
    return out


def reference_colours(rgba):
    """uint8 (n, 3) from updateCol's float colours: min(255, max(0, lrintf(c * 255.0f))), ties to even."""
    c = (np.asarray(rgba, f32)[:, :3] * f32(255)).astype(f32)
    with np.errstate(invalid="ignore"):
        v = np.rint(c)
    v = np.where(np.isfinite(v), v, 0)
    return np.clip(v, 0, 255).astype(np.uint8)


def render(scene, V, pos, rad, dead, colours=None, trail=None):
    """The frame as uint8 [h, w, 3].  colours: None for the plain style, else updateCol's (n, 4) floats (reference
    style).  trail: the centroid ring (slots, 2) as stored (y + 2000), or None."""
    pos, rad = np.asarray(pos, f32).reshape(-1, 2), np.asarray(rad, f32).reshape(-1)
    n = rad.shape[0]
    img = np.full((V.h, V.w, 3), 245, np.uint8)
    for (x1, x2, y1, y2) in scene["rects"]:
        xa, xb, ya, yb = V.px(x2), V.px(x1), V.py(y2), V.py(y1)
        x0, x1p = max(0, int(np.floor(xa))), min(V.w - 1, int(np.ceil(xb)))
        y0, y1p = max(0, int(np.floor(ya))), min(V.h - 1, int(np.ceil(yb)))
        if x0 <= x1p and y0 <= y1p:
            img[y0:y1p + 1, x0:x1p + 1] = 110
    for (x, y, r) in scene["circles"]:
        _paint_disc(img, V, x, y, r, (110, 110, 110))
    _paint_disc(img, V, scene["light_x"], scene["light_y"], scene["light_radius"], (250, 210, 40))
    rgb = plain_colours(rad, dead, scene["min_radius"], scene["max_radius"]) if colours is None \
        else reference_colours(colours)
    if n <= 4096:
        for i in range(n):  # the painter's loop itself
            _paint_disc(img, V, pos[i, 0], pos[i, 1], rad[i], rgb[i])
    elif n:
        _paint_many(img, V, pos, rad, rgb)
    if colours is not None and trail is not None:
        for (x, y) in np.asarray(trail, f32).reshape(-1, 2):
            if x != f32(-5000):
                _paint_disc(img, V, x, f32(y - f32(2000)), scene["centroid_radius"], (255, 0, 0))
    return img


def _paint_many(img, V, pos, rad, rgb):
    """Many small discs: the last bot in index order that covers a pixel is the highest index that covers it.  One
    vectorised pass per offset inside the bounding boxes."""
    cx, cy = V.px(pos[:, 0]), V.py(pos[:, 1])
    pr = (rad * V.scale).astype(f32)
    ok = np.isfinite(cx) & np.isfinite(cy) & np.isfinite(pr)
    cx, cy, pr = np.where(ok, cx, f32(-10)), np.where(ok, cy, f32(-10)), np.where(ok, pr, f32(0))
    (x0, x1), (y0, y1) = _box(V.w, cx, pr), _box(V.h, cy, pr)
    r2 = (pr * pr).astype(f32)
    win = np.zeros(V.h * V.w, np.int64)
    idx = np.arange(1, rad.shape[0] + 1, dtype=np.int64)
    bw, bh = int(np.max(x1 - x0)) + 1, int(np.max(y1 - y0)) + 1
    for j in range(max(bh, 0)):
        yy = y0 + j
        dy = ((yy.astype(f32) + f32(0.5)).astype(f32) - cy).astype(f32)
        dy2 = (dy * dy).astype(f32)
        for i in range(max(bw, 0)):
            xx = x0 + i
            dx = ((xx.astype(f32) + f32(0.5)).astype(f32) - cx).astype(f32)
            m = ok & (xx <= x1) & (yy <= y1) & (((dx * dx).astype(f32) + dy2).astype(f32) <= r2)
            np.maximum.at(win, (yy[m] * V.w + xx[m]), idx[m])
    hit = win > 0
    img.reshape(-1, 3)[hit] = rgb[win[hit] - 1]


def read_ppm(path):
    """(uint8 [h, w, 3], header bytes) of a binary PPM as the frame writers produce it."""
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    assert parts[0] == b"P6" and parts[2] == b"255", parts[:3]
    w, h = (int(t) for t in parts[1].split())
    head = len(data) - 3 * w * h
    assert head == len(b"P6\n%d %d\n255\n" % (w, h))
    return np.frombuffer(data[head:], np.uint8).reshape(h, w, 3), data[:head]
