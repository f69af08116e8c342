"""A numpy statement of cdfo_live_planes (csrc/live.hip): the planes a chunk of live inference reads from its sample rings.  Each
quotient is one correctly rounded fp32 division (numpy's float32 / float32 on the CPU is IEEE), zero padded from H x W to Hp x Wp; a
slot outside the ring names a frame of zeros.  It is what ``StreamingSR.__init__``'s ``plane()`` followed by ``gather_frames`` gives
for the frames the slots hold."""
import numpy as np


def planes(ring: np.ndarray, slots, divisor, Hp: int, Wp: int) -> np.ndarray:
    """ring [cap,H,W] (uint8, uint16 or float32), slots: ring slots -> [len(slots),Hp,Wp] float32 = ring[slot] / divisor, padded."""
    cap, H, W = ring.shape
    out = np.zeros((len(slots), Hp, Wp), np.float32)
    for j, s in enumerate(slots):
        if 0 <= s < cap:
            out[j, :H, :W] = ring[s].astype(np.float32) / np.float32(divisor)
    return out


def live_planes(lr, ufs, pms, rms, win_frame, win_prior, new_frame, new_prior, Hp, Wp, peak):
    """-> x, r, u [K,7,Hp,Wp] and lr_new, p_new, r_new [E,Hp,Wp] of cdfo_live_planes; win_* are [K,7] slot lists, new_* [E]."""
    K = len(win_frame)
    flat = lambda w: [s for row in w for s in row]
    win = lambda a: a.reshape(K, 7, Hp, Wp)
    return (win(planes(lr, flat(win_frame), peak, Hp, Wp)), win(planes(rms, flat(win_prior), peak, Hp, Wp)),
            win(planes(ufs, flat(win_prior), peak, Hp, Wp)), planes(lr, new_frame, peak, Hp, Wp), planes(pms, new_prior, 255, Hp, Wp),
            planes(rms, new_prior, peak, Hp, Wp))
