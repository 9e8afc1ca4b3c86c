"""The numpy statement of the streaming tracker of include/ssba_tracks.h (ssba_track_stream_create / _push / _window): frames
pushed one by one, the state the device keeps restated in numpy.  It is built from the existing statements: features and
matching from tracks_reference, one observation from tracks_refine_reference.  The state is the previous frame's survivors with
their issued ids and (with refinement) the 17 x 17 anchor patch of every survivor's track, the running id, and a ring of the last
`window` frames: per survivor the issued id, the slot of the previous frame it inherited from or -1, the kept flag and the
observation (whole pixel: x, y, d16; refined: u, v, d in 1/256 pixel)."""
import collections

import numpy as np

import tracks_reference as tr
import tracks_refine_reference as rr

PATCH = rr.RADIUS + 1                        # the patch is the 17 x 17 bytes around the anchor: its centre is (8, 8)


class Stream:
    def __init__(self, window, refine=None, **kw):
        self.p = tr.params(**kw)
        self.rp = None if refine is None else rr.refine_params(**refine)
        self.window_frames = int(window)
        self.ring = collections.deque(maxlen=self.window_frames)
        self.prev = None                     # (xy, desc, ids, patches) of the previous frame's survivors, dropped ones included
        self.next_id = 0
        self.pushed = 0
        self.source = None

    def push(self, left, right=None, disp16=None):
        """(ids uint32, uvd float64 (n, 3), num_dropped) of the frame's kept survivors in keypoint order, ids as issued."""
        assert (right is None) != (disp16 is None)
        source = "right" if right is not None else "disp16"
        assert self.source in (None, source)
        self.source = source
        p = self.p
        xy, _, desc = tr.features(left, **p)
        if right is not None:
            rxy, _, rdesc = tr.features(right, **p)
            m, _ = tr.match(desc, xy, rdesc, rxy, tr.GATE_STEREO, **p)
            d16 = np.zeros(len(xy), np.int64)
            d16[m >= 0] = 16 * (xy[m >= 0, 0].astype(np.int64) - rxy[m[m >= 0], 0].astype(np.int64))
        else:
            d16 = np.asarray(disp16).astype(np.int64)[xy[:, 1], xy[:, 0]]
        live = d16 > 0
        xy, desc, d16 = xy[live], desc[live], d16[live]
        n = len(xy)
        ids, source_slot = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        if self.prev is not None:
            pxy, pdesc, pids, _ = self.prev
            m, _ = tr.match(pdesc, pxy, desc, xy, tr.GATE_TEMPORAL, **p)
            a = np.nonzero(m >= 0)[0]
            ids[m[a]] = pids[a]
            source_slot[m[a]] = a
        fresh = np.nonzero(ids < 0)[0]
        ids[fresh] = self.next_id + np.arange(len(fresh))
        self.next_id += len(fresh)
        kept, value, patches = np.ones(n, bool), np.stack([xy[:, 0], xy[:, 1], d16], axis=1).astype(np.int64).reshape(n, 3), None
        if self.rp is not None:
            patches = np.zeros((n, 2 * PATCH + 1, 2 * PATCH + 1), np.uint8)
            for j in range(n):
                x, y = int(xy[j, 0]), int(xy[j, 1])
                patches[j] = self.prev[3][source_slot[j]] if source_slot[j] >= 0 else np.asarray(left)[y - PATCH:y + PATCH + 1, x - PATCH:x + PATCH + 1]
                u, v, d, status = rr.observation(patches[j], PATCH, PATCH, left, right, x, y, d16[j], source_slot[j] < 0, **self.rp)
                value[j] = (u, v, d)
                kept[j] = status == rr.OK
        self.prev = (xy, desc, ids, patches)
        self.ring.append(dict(ids=ids, source=source_slot, kept=kept, value=value))
        self.pushed += 1
        return ids[kept].astype(np.uint32), self._uvd(value[kept]), int((~kept).sum())

    def _uvd(self, value):
        if self.rp is not None:
            return value.astype(np.float64).reshape(-1, 3) / 256.0
        return np.stack([value[:, 0].astype(np.float64), value[:, 1].astype(np.float64), value[:, 2] / 16.0], axis=1).reshape(-1, 3)

    def window(self, frames=None):
        """state_start (frames + 1) uint32, point_id uint32, uvd (N, 3) float64, num_points over the last `frames` pushed frames."""
        frames = min(self.window_frames, self.pushed) if frames is None else int(frames)
        assert 1 <= frames <= min(self.window_frames, self.pushed)
        entries = list(self.ring)[-frames:]
        local, count = [], 0
        for f, e in enumerate(entries):
            mine = np.full(len(e["ids"]), -1, np.int64)
            if f:
                linked = e["source"] >= 0
                mine[linked] = local[f - 1][e["source"][linked]]
            fresh = np.nonzero(mine < 0)[0]
            mine[fresh] = count + np.arange(len(fresh))
            count += len(fresh)
            local.append(mine)
        length = np.zeros(count, np.int64)
        for mine, e in zip(local, entries):
            np.add.at(length, mine[e["kept"]], 1)
        keep = length >= self.p["min_track_length"]
        renamed = np.cumsum(keep) - 1
        start, out_ids, out_uvd = [0], [], []
        for mine, e in zip(local, entries):
            k = e["kept"] & keep[mine] if len(mine) else np.zeros(0, bool)
            out_ids.append(renamed[mine[k]] if len(mine) else np.zeros(0, np.int64))
            out_uvd.append(self._uvd(e["value"][k]))
            start.append(start[-1] + int(k.sum()))
        return np.array(start, np.uint32), np.concatenate(out_ids).astype(np.uint32), np.concatenate(out_uvd).reshape(-1, 3), int(keep.sum())
