"""Which frames of a clip are key frames.

The reference takes a key frame at `idx % interval == 0` and at no other time (demo.py:235).  On real video that rule warps the
features of the old scene onto the new one for up to interval - 1 frames after a cut, and pays the full trunk every `interval`
frames on a still camera.  KeySchedule.adaptive decides from a measure of how much the frame differs from the last key frame,
made on the GPU where the frame already is (accel_model_frame_change: the share of cell x cell cells whose mean absolute change
exceeds `level` grey levels).

A schedule is asked once per frame, in order: `decide(idx, change)` -> bool, where `change` is None (nothing to compare with yet)
or a list of (changed, cells, sad) per frame of the call.  The schedules that do not look at the frame say so with
`needs_change = False` and are never given one.
"""


class KeySchedule(object):
    needs_change = False

    def __init__(self, rule, **kw):
        self._rule = rule
        self.__dict__.update(kw)
        self.last_key = None      # index of the last key frame decided

    # -- the three kinds ---------------------------------------------------------------------------
    @classmethod
    def fixed(cls, interval):
        """the reference's rule: a key frame at idx % interval == 0"""
        interval = int(interval)
        if interval < 1:
            raise ValueError("interval = %d, must be >= 1" % interval)
        return cls("fixed", interval=interval)

    @classmethod
    def explicit(cls, keys):
        """key frames at exactly the indices in `keys` (frame 0 must be one: a clip starts with a key frame)"""
        keys = frozenset(int(k) for k in keys)
        if 0 not in keys:
            raise ValueError("an explicit schedule must hold frame 0: there is no feature to propagate before the first key frame")
        return cls("explicit", keys=keys)

    @classmethod
    def adaptive(cls, share, level=16.0, cell=32, max_interval=5, min_interval=1):
        """a key frame at frame 0, when max_interval frames have passed since the last key frame, and when ANY frame of the call has
        changed / cells > share (strict) while at least min_interval frames have passed.  level: grey levels of mean absolute change
        above which a cell counts as changed; cell: 8, 16, 32 or 64 pixels"""
        from ..utils.image import FRAME_CELLS, frame_level_q
        share = float(share)
        if not 0.0 <= share <= 1.0:
            raise ValueError("share = %r, must be in 0 .. 1" % (share,))
        if int(cell) not in FRAME_CELLS:
            raise ValueError("cell = %r, must be one of %s" % (cell, ", ".join(str(c) for c in FRAME_CELLS)))
        max_interval, min_interval = int(max_interval), int(min_interval)
        if max_interval < 1 or min_interval < 1 or min_interval > max_interval:
            raise ValueError("min_interval = %d and max_interval = %d, must be 1 <= min_interval <= max_interval" % (min_interval, max_interval))
        s = cls("adaptive", share=share, level=float(level), level_q=frame_level_q(level), cell=int(cell), max_interval=max_interval,
                min_interval=min_interval)
        s.needs_change = True
        return s

    # -- the decision ------------------------------------------------------------------------------
    def decide(self, idx, change=None):
        """whether frame `idx` is a key frame; frames are asked in order, once each"""
        idx = int(idx)
        if self._rule == "fixed":
            key = idx % self.interval == 0
        elif self._rule == "explicit":
            key = idx in self.keys
        else:
            since = None if self.last_key is None else idx - self.last_key
            if since is None or since <= 0 or change is None:       # the first frame, a new clip (indices start over), nothing kept to compare with
                key = True
            elif since >= self.max_interval:
                key = True
            else:
                key = since >= self.min_interval and any(int(c) > self.share * int(cells) for c, cells, _ in change)
        if key:
            self.last_key = idx
        return bool(key)

    def __repr__(self):
        if self._rule == "fixed":
            return "KeySchedule.fixed(%d)" % self.interval
        if self._rule == "explicit":
            return "KeySchedule.explicit(%s)" % sorted(self.keys)
        return "KeySchedule.adaptive(share=%g, level=%g, cell=%d, max_interval=%d, min_interval=%d)" % (
            self.share, self.level, self.cell, self.max_interval, self.min_interval)
