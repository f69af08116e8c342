// The image map: where the images of a pixel-major fp32 operand [M][P][ld >= 64] lie when they are not one dense block.
// Image m starts at  first + (m % Bi) * s_b + (m / Bi) * s_g  floats (the form pc_plane uses for the prior planes); inside an image
// nothing changes: pixel pitch ld, dense pixels.  A neighbour group reads its frames out of the clip-major feature stack this way
// (Bi = B, s_b = 7 P 64, s_g = P 64) instead of from a frame-major copy.  The dense case is never expressed as a map inside a
// kernel: it is the instantiation without one, whose instructions stay what they were.
#pragma once

struct im_map {
  int Bi; long long s_b, s_g;
};

// a map a kernel may take: strides that keep every image 16-byte aligned
inline bool im_map_ok(const im_map& m) { return m.Bi > 0 && m.s_b >= 0 && m.s_g >= 0 && m.s_b % 4 == 0 && m.s_g % 4 == 0; }

// the dense stack [M][P][ld] as a map (an operand without a map of its own inside a mapped launch)
inline im_map im_dense(int M, long long P, int ld) { return im_map{M > 0 ? M : 1, P * ld, 0}; }

// floats from the first image to image m
__host__ __device__ __forceinline__ long long im_offset(const im_map& mp, int m) {
  return (long long)(m % mp.Bi) * mp.s_b + (long long)(m / mp.Bi) * mp.s_g;
}
