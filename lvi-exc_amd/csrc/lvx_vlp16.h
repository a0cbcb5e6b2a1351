// lvx_vlp16.h — VLP-16 scan ingestion, host- and device-callable: licalib::VelodyneCorrection::unpack_scan (src/lvi_exc/include/utils/vlp_common.h:51-149), its
// range test (:252-255), its time table (:179-181, 244-248), its constants and row permutation (:184-242) and the organised overload (:152-176), called per scan from
// LioDataset::read (dataset_reader.h:152-157).  k_vlp16_unpack / k_vlp16_organised of lvx_upstream.hip call vlp16_point / vlp16_time one lane per record;
// tests/native/vlp16_host_check.cpp builds the same functions with g++ (-ffp-contract=off, as lvx_upstream.hip is built) and the suites compare records byte for byte.
//
// One record from (packet bytes, block, firing, dsr, block_counter, scan stamp), in the reference's arithmetic type for type:
//   packet      1206 bytes: 12 blocks of {uint16 header, uint16 rotation, 32 x {uint16 distance, uint8 intensity}}, then 6 trailer bytes; all little-endian
//   azimuth     (float)rotation[block];  azimuth_diff = (float)((36000 + rotation[block + 1] - rotation[block]) % 36000) in int for blocks 0 .. 10 (C's truncating %),
//               block 11 reuses the diff of block 10 of ITS packet (last_azimuth_diff is reset per packet, :69)
//   corrected   azimuth + (azimuth_diff * ((dsr * 2.304f) + (firing * 55.296f)) / 110.592f) in float without contraction; ((int)round(.)) % 36000 indexes the rotation
//               tables.  The index can be NEGATIVE in one corner: raw rotations are never reduced, so a rotation above 36000 in block 10 followed by a small one
//               in block 11 gives block 11 a negative diff on a small azimuth.  With min_angle >= 0 and min_angle < max_angle the window test drops such a point
//               before the tables are read; with a wrapped window the reference would read in front of its tables (undefined) — here the point is outside the
//               window in both cases.
//   position    distance = raw_u16 * 0.002f;  x = distance * cos_vert[dsr] * sin_rot, y = distance * cos_vert[dsr] * cos_rot, z = distance * sin_vert[dsr]; stored (y, -x, z)
//   intensity   (float)data[k + 2]
//   range       the float distance against the DOUBLE bounds (:252-255): outside them x = y = z = NAN, intensity 0, the timestamp still written
//   placement   row scan_mapping_16[dsr], column 2 * block_counter + firing; block_counter runs over the whole scan
//   timestamp   scan_stamp + (row * 2.304 * 1e-6 + column * 55.296 * 1e-6) in double, the table of :246 indexed with the MAPPED row as :127 does (the reference's quirk)
//   window      a point whose corrected azimuth lies outside [min_angle, max_angle] (or, with min > max, inside (max, min)) is not written by the reference and stays
//               value-initialised: 32 zero bytes
//   headers     never checked (the reference does not); vlp16_bad_header lets the caller count the blocks that are not 0xEEFF
// The pad fields of a record are written as zero, so records compare as bytes.
//
// THE TABLES are built on the HOST by vlp16_build_tables, once per context, with libm's cosf / sinf, exactly as setParameters does (:191-195, 205-226), and uploaded;
// no kernel evaluates a device cosine: another implementation of cosf need not round as libm's does (numpy's float32 cosine differs from it at 6301 of the 36000
// entries, and even float(cos(double)) at 488), and one different table entry is a different point.  angles::from_degrees is not
// part of the reference tree; it is restated here from its public definition in ros/angles (angles.h: `return degrees * M_PI / 180.0;` on a double).
//
// DEVIATION (the one): the reference sizes every cloud to its own 24 x packets columns; the context keeps one width W for all scans, so the columns beyond
// 24 x packets of a shorter scan hold "no return": x = y = z = NAN, intensity 0, timestamp 0 (vlp16_padding).  The association skips NaN, the emission timestamp 0.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef LVX_HD
#if defined(__HIPCC__)
#define LVX_HD __host__ __device__ __forceinline__
#else
#define LVX_HD inline
#endif
#endif

namespace lvx {

#define LVX_VLP16_BYTES 1206          // one packet
#define LVX_VLP16_BLOCKS 12           // BLOCKS_PER_PACKET
#define LVX_VLP16_COLS 24             // columns one packet fills: 2 firings per block
#define LVX_VLP16_ROWS 16
#define LVX_VLP16_ROT 36000           // ROTATION_MAX_UNITS
#define LVX_VLP16_MAX_PACKETS 76      // mVLP16TimeBlock has 1824 = 24 x 76 columns (:320)
#define LVX_VLP16_MAX_W 1824

struct VlpPoint { float x, y, z, pad; float intensity; float pad2; double timestamp; };   // lvx_point_xyzit
struct VlpOptions { double min_range, max_range; int32_t min_angle, max_angle; };          // lvx_vlp16_options
struct VlpTables { const float* cos_rot; const float* sin_rot; const float* cos_vert; const float* sin_vert; };   // [36000], [36000], [16], [16]
enum { VLP_IN_RANGE = 0, VLP_OUT_OF_RANGE = 1, VLP_OUTSIDE_WINDOW = 2 };

// scan_mapping_16 (:227-242) and its inverse
LVX_HD int vlp16_row_of_dsr(int dsr) { return (dsr & 1) ? 7 - (dsr >> 1) : 15 - (dsr >> 1); }
LVX_HD int vlp16_dsr_of_row(int row) { return row >= 8 ? 2 * (15 - row) : 2 * (7 - row) + 1; }
LVX_HD int vlp16_u16(const uint8_t* p) { return (int)p[0] | ((int)p[1] << 8); }
LVX_HD bool vlp16_bad_header(const uint8_t* packet, int block) { return vlp16_u16(packet + 100 * block) != 0xeeff; }
// mVLP16TimeBlock[w][h] (:244-248; h and w are unsigned there)
LVX_HD double vlp16_time(int h, int w) { return (double)(unsigned)h * 2.304 * 1e-6 + (double)(unsigned)w * 55.296 * 1e-6; }
LVX_HD VlpPoint vlp16_zero() { VlpPoint p; p.x = p.y = p.z = p.pad = p.intensity = p.pad2 = 0.f; p.timestamp = 0.0; return p; }
LVX_HD VlpPoint vlp16_padding() { VlpPoint p = vlp16_zero(); p.x = p.y = p.z = NAN; return p; }

// One record of unpack_scan (:76-147).  packet: the 1206 bytes; block_counter: 12 x (the packet's index in its scan) + block.  Returns VLP_*; *row and *col say where
// the record belongs, whatever the return value.
LVX_HD int vlp16_point(const uint8_t* packet, int block, int firing, int dsr, int block_counter, double scan_stamp, const VlpTables& T, const VlpOptions& o, VlpPoint* out,
                       int* row, int* col) {
  const int rot = vlp16_u16(packet + 100 * block + 2);
  const int b0 = block < LVX_VLP16_BLOCKS - 1 ? block : LVX_VLP16_BLOCKS - 2;   // block 11: last_azimuth_diff = the diff of block 10
  const int r0 = vlp16_u16(packet + 100 * b0 + 2), r1 = vlp16_u16(packet + 100 * (b0 + 1) + 2);
  const float azimuth = (float)rot;
  const float azimuth_diff = (float)((36000 + r1 - r0) % 36000);
  const float azimuth_corrected_f = azimuth + (azimuth_diff * ((dsr * 2.304f) + (firing * 55.296f)) / 110.592f);
  const int azimuth_corrected = ((int)roundf(azimuth_corrected_f)) % 36000;
  *row = vlp16_row_of_dsr(dsr);
  *col = 2 * block_counter + firing;
  *out = vlp16_zero();
  const bool inside = (azimuth_corrected >= o.min_angle && azimuth_corrected <= o.max_angle && o.min_angle < o.max_angle) ||
                      (o.min_angle > o.max_angle && (azimuth_corrected <= o.max_angle || azimuth_corrected >= o.min_angle));
  if (!inside || azimuth_corrected < 0) return VLP_OUTSIDE_WINDOW;
  const uint8_t* d = packet + 100 * block + 4 + 3 * (16 * firing + dsr);
  const float distance = vlp16_u16(d) * 0.002f;
  const float cos_vert_angle = T.cos_vert[dsr], sin_vert_angle = T.sin_vert[dsr];
  const float cos_rot_angle = T.cos_rot[azimuth_corrected], sin_rot_angle = T.sin_rot[azimuth_corrected];
  const float x = distance * cos_vert_angle * sin_rot_angle;
  const float y = distance * cos_vert_angle * cos_rot_angle;
  const float z = distance * sin_vert_angle;
  out->timestamp = scan_stamp + vlp16_time(*row, *col);
  if (distance >= o.min_range && distance <= o.max_range) {   // float against double, as pointInRange
    out->x = y; out->y = -x; out->z = z; out->intensity = (float)d[2];
    return VLP_IN_RANGE;
  }
  out->x = out->y = out->z = NAN;
  return VLP_OUT_OF_RANGE;
}

// One record of unpack_scan's second overload (:152-176): the point copied, its time = timebase + table[w][h]
LVX_HD VlpPoint vlp16_organised_point(const float* xyzi, int h, int w, double timebase) {
  VlpPoint p = vlp16_zero();
  p.x = xyzi[0]; p.y = xyzi[1]; p.z = xyzi[2]; p.intensity = xyzi[3];
  p.timestamp = timebase + vlp16_time(h, w);
  return p;
}

// The width of the organised result.  offsets[n_scans + 1]: non-decreasing packet offsets.  W_in = 0: 24 x the longest scan.  Returns 0, or 1 = bad offsets,
// 2 = a scan longer than the time table (76 packets), 3 = W_in smaller than the longest scan needs.
inline int vlp16_width(int n_scans, const int32_t* offsets, int W_in, int* W) {
  int longest = 0;
  if (n_scans > 0 && offsets[0] < 0) return 1;
  for (int s = 0; s < n_scans; ++s) {
    if (offsets[s + 1] < offsets[s]) return 1;
    const int np = offsets[s + 1] - offsets[s];
    if (np > LVX_VLP16_MAX_PACKETS) return 2;
    if (np > longest) longest = np;
  }
  if (W_in < 0 || (W_in > 0 && W_in < LVX_VLP16_COLS * longest)) return 3;
  *W = W_in > 0 ? W_in : LVX_VLP16_COLS * longest;
  return 0;
}

// setParameters (:191-195, 205-226), HOST ONLY.  The arguments reach libm through volatiles: a compiler that sees a constant argument folds cosf itself, and its
// folding is correctly rounded where libm's cosf need not be.
inline void vlp16_build_tables(float* cos_rot, float* sin_rot, float* cos_vert, float* sin_vert) {
  for (uint16_t rot_index = 0; rot_index < LVX_VLP16_ROT; ++rot_index) {
    const double degrees = 0.01f * rot_index;                                  // ROTATION_RESOLUTION * rot_index in float, widened by from_degrees' parameter
    volatile float rotation = (float)(degrees * 3.14159265358979323846 / 180.0);   // angles::from_degrees, narrowed by `float rotation =`
    cos_rot[rot_index] = cosf(rotation);
    sin_rot[rot_index] = sinf(rotation);
  }
  static const double vert_correction[16] = {-0.2617993877991494, 0.017453292519943295, -0.22689280275926285, 0.05235987755982989, -0.19198621771937624, 0.08726646259971647,
                                             -0.15707963267948966, 0.12217304763960307, -0.12217304763960307, 0.15707963267948966, -0.08726646259971647, 0.19198621771937624,
                                             -0.05235987755982989, 0.22689280275926285, -0.017453292519943295, 0.2617993877991494};
  for (int i = 0; i < 16; ++i) {
    volatile float v = (float)vert_correction[i];   // float vert_correction[16] = {double constants}
    cos_vert[i] = cosf(v);                          // std::cos(float) is cosf
    sin_vert[i] = sinf(v);
  }
}

}  // namespace lvx
