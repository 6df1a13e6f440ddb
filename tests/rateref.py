"""The rule of the frame-rate conversion, restated from its text in plain Python integers (no numpy in the rule): which output pictures an
input's pts yields, with which tick pts and weights.  Python's integers are unbounded, so nothing here can overflow: the C plan (rate_host.c, 128-bit
products) is compared against this step for step.  `mix` is the sample rule of a blended picture; `shown` turns a sequence of inputs into the pictures the ticks show."""

OFF, HOLD, BLEND = 0, 1, 2


class Plan:
    """pps: pts units per second.  D = pps * fps_den, N = fps_num; tick k lies at T0 + k D / N, its pts is T0 + floor(k D / N)."""

    def __init__(self, mode, pps, fps_num, fps_den=1, max_fill=2, t0=None, k_next=0):
        self.mode, self.N, self.D, self.max_fill = mode, fps_num, pps * fps_den, max_fill
        self.t0, self.k_next = t0, k_next  # t0 None: the first input anchors the grid
        self.prev = None if t0 is None else (t0 + (k_next - 1) * self.D // self.N if k_next > 0 else t0)

    def tick_pts(self, k):
        return self.t0 + k * self.D // self.N

    def _anchor(self, p):
        self.t0, self.k_next = p, 1
        return [p], [256]

    def weight(self, k, p0, p1):
        """round-half-up(256 (T_k - p0) / (p1 - p0)) clamped to 0 .. 256, T_k the exact rational"""
        if p1 <= p0:
            return 256
        num = 256 * ((self.t0 - p0) * self.N + k * self.D)  # 256 (T_k - p0) N
        den = (p1 - p0) * self.N
        return min(max((2 * num + den) // (2 * den), 0), 256)

    def step(self, p):
        """-> (out_pts, weights, resync).  hold: weight 0 = the previous output picture again, 256 = the input.  blend: the weight of the input against the
        previous input."""
        if self.t0 is None:
            out = self._anchor(p) + (False,)
        elif p < self.prev:
            out = self._anchor(p) + (True,)
        else:
            tol = 2 if self.mode == HOLD else 16
            k_max = (tol * self.N * (p - self.t0) + self.D) // (tol * self.D)
            n = k_max - self.k_next + 1
            if n <= 0:
                out = ([], [], False)
            elif n - 1 > self.max_fill:
                out = self._anchor(p) + (True,)
            else:
                ks = range(self.k_next, k_max + 1)
                ws = [256 if k == k_max else 0 for k in ks] if self.mode == HOLD else [self.weight(k, self.prev, p) for k in ks]
                out = ([self.tick_pts(k) for k in ks], ws, False)
                self.k_next = k_max + 1
        self.prev = p
        return out


def run(mode, pps, fps_num, fps_den, max_fill, pts_list):
    """the whole sequence: a list of (out_pts, weights, resync) per input"""
    pl = Plan(mode, pps, fps_num, fps_den, max_fill)
    return [pl.step(p) for p in pts_list]


def shown(mode, steps):
    """What every output picture shows, from run()'s result: a list of (tick pts, a, b, w) -- the picture is mix(input a, input b, w), a and b input indices.
    hold: a repeat shows the input of the previous output picture (w = 256 on that index)."""
    out, last, prev_in = [], None, None
    for i, (pts, ws, _) in enumerate(steps):
        for t, w in zip(pts, ws):
            if mode == HOLD:
                src = i if w == 256 else last
                out.append((t, src, src, 256))
                last = src
            else:
                out.append((t, i if prev_in is None else prev_in, i, w))
        prev_in = i
    return out


def mix(a, b, w):
    """(a (256 - w) + b w + 128) >> 8 per sample (uint8 numpy arrays)"""
    import numpy as np
    return ((a.astype(np.uint32) * (256 - w) + b.astype(np.uint32) * w + 128) >> 8).astype(np.uint8)
