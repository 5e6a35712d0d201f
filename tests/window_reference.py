"""The restatement of include/ba_window.h in numpy: covisibility with a query frame, the choice of a
local bundle-adjustment window, the gather of that window into mv_ba_solve_dev's layout and the
scatter of its poses, written for reading -- one sequence at a time, integers and bit-for-bit copies
only.  The GPU tests require the kernels (csrc/hip/k_bawin.hip) to equal these functions exactly.
"""
import numpy as np

import tracks_reference as tr

MV_OK, MV_ERR_CAPACITY = tr.MV_OK, tr.MV_ERR_CAPACITY
BA_MAX_POSES = 16
DEFAULTS = dict(min_shared=15, n_fixed=2, min_obs=2)
IDENTITY_POSE = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
UNIT_CAMERA = np.array([1, 1, 0, 0], np.float32)

_clamp = tr._clamp


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def counting(track_id_s, num_tracks_s, flags_s, f_count):
    """One sequence: track_id [F][cap], ldmk_flags [track_cap] -> bool [F][cap], the slots that count:
    f < f_count, t = track_id in [0, T) and ldmk_flags[t] == 0."""
    F, cap = track_id_s.shape
    T = _clamp(num_tracks_s, len(flags_s))
    out = np.zeros((F, cap), bool)
    for f in range(min(f_count, F)):
        t = track_id_s[f].astype(np.int64)
        ok = (t >= 0) & (t < T)
        ok[ok] = flags_s[t[ok]] == 0
        out[f] = ok
    return out


def _f_count(F, f_count):
    f_count = F if f_count is None else int(f_count)
    assert 1 <= f_count <= F
    return f_count


def covisibility(track_id, num_tracks, status, ldmk_flags, f_q, f_count=None):
    """track_id [B][F][cap], num_tracks / status / f_q [B], ldmk_flags [B][track_cap] -> covis [B][F]"""
    B, F, cap = track_id.shape
    f_count = _f_count(F, f_count)
    covis = np.zeros((B, F), np.int32)
    for s in range(B):
        fq = int(f_q[s])
        if status[s] != MV_OK or fq < 0 or fq >= f_count:
            continue
        cnt = counting(track_id[s], num_tracks[s], ldmk_flags[s], f_count)
        Q = set(track_id[s, fq][cnt[fq]].tolist())
        for f in range(f_count):
            covis[s, f] = sum(1 for t in track_id[s, f][cnt[f]].tolist() if t in Q)
    return covis


def select(covis, f_q, status, W, f_count=None, eligible=None, p=None):
    """covis [B][F], f_q / status [B], eligible [B][F] or None -> dict(win_frames [B][W], win_count [B],
    pose_fixed [B][W])"""
    p = params(**(p or {}))
    B, F = covis.shape
    f_count = _f_count(F, f_count)
    assert 1 <= W <= BA_MAX_POSES
    out = dict(win_frames=np.full((B, W), -1, np.int32), win_count=np.zeros(B, np.int32),
               pose_fixed=np.ones((B, W), np.int32))
    for s in range(B):
        fq = int(f_q[s])
        if status[s] != MV_OK or fq < 0 or fq >= f_count:
            continue
        cand = [f for f in range(f_count) if f != fq and (eligible is None or eligible[s, f] != 0) and
                int(covis[s, f]) >= p["min_shared"]]
        cand.sort(key=lambda f: (int(covis[s, f]), f), reverse=True)  # greater covis, ties to the greater f
        win = sorted(cand[:W - 1] + [fq])
        out["win_count"][s] = len(win)
        held = 0
        for k, f in enumerate(win):
            out["win_frames"][s, k] = f
            fixed = f != fq and held < p["n_fixed"]
            held += f != fq
            out["pose_fixed"][s, k] = 1 if fixed else 0
    return out


def factors(kp, poses, cameras, track_id, num_tracks, ldmk_flags, win_frames, factor_cap, f_count=None, p=None):
    """kp [B][F][cap][2], poses [B][F][7], cameras [B][F][4] float32, the map state and win_frames [B][W]
    -> dict(win_obs [B][track_cap], ldmk_id, pose_id [stored], meas [stored][2], pose_offsets [B*W + 1],
    status, poses_w [B][W][7], cameras_w [B][W][4]), stored = min(total, factor_cap)."""
    p = params(**(p or {}))
    B, F, cap = track_id.shape
    track_cap = ldmk_flags.shape[1]
    W = win_frames.shape[1]
    f_count = _f_count(F, f_count)
    win_obs = np.zeros((B, track_cap), np.int32)
    poses_w = np.tile(IDENTITY_POSE, (B, W, 1))
    cameras_w = np.tile(UNIT_CAMERA, (B, W, 1))
    lid, pid, meas = [], [], []
    off = np.zeros(B * W + 1, np.int32)
    total = 0
    for s in range(B):
        cnt = counting(track_id[s], num_tracks[s], ldmk_flags[s], f_count)
        used = [k for k in range(W) if 0 <= int(win_frames[s, k]) < f_count]
        for k in used:
            f = int(win_frames[s, k])
            for t in track_id[s, f][cnt[f]].tolist():
                win_obs[s, t] += 1
            poses_w[s, k], cameras_w[s, k] = poses[s, f], cameras[s, f]
        for k in range(W):
            if used and k not in used:
                cameras_w[s, k] = cameras[s, int(win_frames[s, used[0]])]
            off[s * W + k] = total
            if k not in used:
                continue
            f = int(win_frames[s, k])
            for i in range(cap):
                if not cnt[f, i]:
                    continue
                t = int(track_id[s, f, i])
                if win_obs[s, t] < p["min_obs"]:
                    continue
                if total < factor_cap:
                    lid.append(s * track_cap + t)
                    pid.append(s * W + k)
                    meas.append(kp[s, f, i])
                total += 1
    off[B * W] = total
    return dict(win_obs=win_obs, ldmk_id=np.array(lid, np.int32), pose_id=np.array(pid, np.int32),
                meas=np.array(meas, np.float32).reshape(-1, 2), pose_offsets=off,
                status=MV_ERR_CAPACITY if total > factor_cap else MV_OK, poses_w=poses_w, cameras_w=cameras_w)


def scatter(poses, win_frames, poses_w, f_count=None):
    """poses [B][F][7] with poses_w [B][W][7] written into the window's frames -> a new array"""
    B, F = poses.shape[:2]
    f_count = _f_count(F, f_count)
    out = poses.copy()
    for s in range(B):
        for k in range(win_frames.shape[1]):
            f = int(win_frames[s, k])
            if 0 <= f < f_count:
                out[s, f] = poses_w[s, k]
    return out


def ba_batch(fa, landmarks, win):
    """factors()'s output, landmarks [B][track_cap][3] and select()'s output as the batch dict of
    lba_reference.solve_batch (F = W)"""
    B, W = win["win_frames"].shape
    return dict(F=W, track_cap=landmarks.shape[1], poses=fa["poses_w"], landmarks=landmarks,
                cameras=fa["cameras_w"], ldmk_id=fa["ldmk_id"], pose_id=fa["pose_id"], meas=fa["meas"],
                pose_offsets=fa["pose_offsets"], pose_fixed=win["pose_fixed"])


def local_ba_scene(seed, F=24, cap=64, first_perturbed=19, sigma_rot=0.005, sigma_t=0.05):
    """The long-map scene of the local-BA tests: test_gpu_tracks.make_case(seed, 1, F, cap, p_link=0.85,
    p_conflict=0, hostile=False), more frames than mv_ba_solve_dev accepts.  Frames first_perturbed ..
    F - 1 are perturbed as lba_reference.ba_scene perturbs (through the retraction, N(0, sigma_rot) rad
    and N(0, sigma_t) per axis); landmarks are triangulated from the perturbed poses with max_reproj_px
    huge and the tracks the true poses flag MV_LDMK_REPROJ are dropped."""
    import lba_reference as lr
    import test_gpu_tracks as tg

    case = tg.make_case(seed, 1, F, cap, p_link=0.85, p_conflict=0.0, hostile=False)
    rng = np.random.default_rng(seed + 1000)
    true = case["poses"].copy()
    pert = true.copy()
    for f in range(first_perturbed, F):
        d = np.concatenate([rng.normal(0, sigma_rot, 3), rng.normal(0, sigma_t, 3)])
        pert[0, f] = lr.retract_pose(true[0, f], d).astype(np.float32)
    track_cap = F * cap
    lk = tr.link(case["n"], case["idx"], case["score"], 2, track_cap)
    _, flags_true = tr.triangulate(true, case["cams"], case["kp"], case["idx"], lk)
    ldmk, flags = tr.triangulate(pert, case["cams"], case["kp"], case["idx"], lk, max_reproj=1e30)
    flags = flags | (flags_true & tr.REPROJ)
    return dict(case=case, lk=lk, poses_true=true, poses=pert, landmarks=ldmk, ldmk_flags=flags, track_cap=track_cap)
