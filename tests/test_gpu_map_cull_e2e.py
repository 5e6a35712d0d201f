"""GPU: the two scenes of tests/mapcull_reference.py end to end on the device -- one wrong observation
taken out and its landmark rescued; a map that stays within track_cap by stale, cull and compact where
the plain run ends in MV_ERR_CAPACITY -- with the state, landmarks and flags equal to the
restatement's, bit for bit, after every step."""
import numpy as np
import pytest

import mapcull_reference as cl
from test_gpu_map_correct import on_stream
from test_gpu_map_cull import DeviceCull
from test_gpu_map_update import dev_of
from test_mapcull_reference import check_rescue, statuses

pytestmark = pytest.mark.gpu


class DeviceOps:
    """the stages of mapcull_reference's flows on the device: the new calls and the existing
    map_extend and map_triangulate.  Every stage loads the map into fresh guarded buffers and writes
    the device's result back into st, ldmk and flags."""

    def __init__(self, ctx, torch):
        self.ctx, self.torch = ctx, torch

    def _back(self, dm, st, ldmk, flags):
        ds, dl, df = dm.map()
        for k, v in ds.items():
            st[k][...] = v
        ldmk[...], flags[...] = dl, df

    def triangulate(self, poses, cams, kp, st, ldmk, flags, f_count=None, select=None):
        t = dev_of(self.torch)
        dm = DeviceCull(self.torch, st, ldmk, flags)
        with on_stream(self.ctx, self.torch):
            dm.triangulate(self.ctx, t(poses), t(cams), t(kp), f_count=f_count, select=t(select))
        self._back(dm, st, ldmk, flags)

    def screen(self, poses, cams, kp, st, ldmk, flags, f_count=None, p=None):
        return DeviceCull(self.torch, st, ldmk, flags).screen(self.ctx, (poses, cams, kp), f_count=f_count, p=p)

    def stale(self, st, flags, f_count=None, p=None):
        L = flags.shape[1]
        return DeviceCull(self.torch, st, np.zeros((1, L, 3), np.float32), flags).stale(self.ctx, f_count=f_count, p=p)

    def cull(self, st, ldmk, flags, remove, drop, f_count=None, p=None):
        dm = DeviceCull(self.torch, st, ldmk, flags)
        out = dm.cull(self.ctx, remove, drop, f_count=f_count, p=p)
        self._back(dm, st, ldmk, flags)
        return out

    def compact(self, st, ldmk, flags):
        dm = DeviceCull(self.torch, st, ldmk, flags)
        out = dm.compact(self.ctx)
        self._back(dm, st, ldmk, flags)
        return out

    def extend(self, st, f_new, n_prev, n_new, idx):
        t = dev_of(self.torch)
        L = st["track_first"].shape[1]
        dm = DeviceCull(self.torch, st, np.zeros((1, L, 3), np.float32), np.zeros((1, L), np.int32))
        with on_stream(self.ctx, self.torch):
            dm.extend(self.ctx, f_new, t(np.ascontiguousarray(n_prev)), t(np.ascontiguousarray(n_new)),
                      t(np.ascontiguousarray(idx)), None)
        for k, v in dm.state().items():
            st[k][...] = v
        return dm.outputs()


def test_rescue(ctx, torch_cuda):
    rs = cl.rescue_scene()
    cpu = cl.rescue_flow(rs)
    dev = cl.rescue_flow(rs, ops=DeviceOps(ctx, torch_cuda))
    cl.same_records(cpu[3], dev[3])
    check_rescue(rs, *dev)


def test_bounded_map(ctx, torch_cuda):
    bc = cl.bounded_case()
    ops = DeviceOps(ctx, torch_cuda)
    for culled in (True, False):
        cpu = cl.bounded_flow(bc, cl.BOUND_TRACK_CAP, culled=culled)
        dev = cl.bounded_flow(bc, cl.BOUND_TRACK_CAP, culled=culled, ops=ops)
        cl.same_records(cpu[3], dev[3])
        if culled:  # the map stays within track_cap
            assert all(s == 0 for s in statuses(dev[3])) and int(dev[0]["num_tracks"][0]) <= cl.BOUND_TRACK_CAP
        else:  # what users meet today
            assert statuses(dev[3])[-1] == cl.MV_ERR_CAPACITY
