// The drawing end of the video node on the device for gfx950: the car box of cv2_add_bbox (yolo_modules/yolo_cv.py:239-270), the plate
// edges and the inverse map of the clipped plate of ProjectRectangle6D.add_edges (licence_plate_render/__init__.py:379-402), and the
// NMS boxes, from the rows where the detection kernels left them:
//   overlay_shapes_kernel   one thread per (image, slot): the slot's four integer vertices, colour, thickness and enabled flag; the
//                           plate's thread also solves the 8 x 8 system of the plate-image -> frame homography (fp64 Gaussian
//                           elimination with partial pivoting) and writes the (9) fp32 matrix yolo_warp_u8_to_nchw reads, and lp_valid
//   overlay_labels_kernel   one thread per (image, slot): the slot's label -- [name ' '] score [' ' degrees] as text bytes, placed over
//                           the box's top-left corner and moved inside the frame (integers only)
//   overlay_text_kernel     one block per tile of one LABEL's rectangle (not of the frame): bitmap-font text and its ground box
//   overlay_draw_kernel     one block per 256 x 32 pixel tile of one image: the image's 4 K segments go to LDS with their
//                           t/2-expanded bounding boxes, wave 0 compacts those that meet the tile (ballot + popcount: ordered, no
//                           atomics), and each thread tests its pixels against the list from the highest slot down -- the first hit is
//                           the colour.  The distance rule is exact integer arithmetic (include/yolo_amd.h, yolo_overlay_draw).
// Compiled with -ffp-contract=off: the shapes are the op-by-op fp64 / fp32 definition of the header, tests/overlay_ref.py restates it.
// The draw kernel reads no frame byte and stores only painted pixels (byte stores: the frame may start at any address); a tile no
// segment meets leaves after the compaction, so an image without an enabled shape is never addressed.
#include "common.h"
#include <float.h>

constexpr int OV_SLOT_WORDS = YOLO_OVERLAY_SLOT_WORDS;  // x0 y0 x1 y1 x2 y2 x3 y3 colour thickness enabled pad
constexpr int OV_MAX_K = YOLO_OVERLAY_MAX_SLOTS;
constexpr int OV_MAX_SEG = OV_MAX_K * 4;
constexpr int OV_MAX_C = 4;
constexpr int OV_MAX_SIDE = 16384;
constexpr int OV_MAX_COORD = 1 << 20;
constexpr int OV_MAX_T = 255;                           // t^2 (d.d) <= 2^16 * 2^43 stays far inside 64 bits
constexpr int OV_THREADS = 256;
constexpr int OV_RUN = 4;                               // adjacent pixels a thread owns in a row
constexpr int OV_TILE_W = 64 * OV_RUN;                  // one wave spans a tile row
constexpr int OV_WAVE_ROWS = 8;                         // rows a wave owns
constexpr int OV_TILE_H = 4 * OV_WAVE_ROWS;             // 4 waves
constexpr int OV_SHAPE_THREADS = 64;

// ---- shapes ---------------------------------------------------------------------------------------------------------------------

struct OverlayShapesArgs {
    const float* rows; const int* kept; const int* kept_count; int nbox, rows_C, post_nms, cand_per_box;
    const unsigned char* palette; int npalette;
    const float* pred; int pred_C; float car_threshold; int use_r; unsigned car_color;
    const float* lp; double fx, fy, cx, cy; int cam_w, cam_h; float lp_threshold; unsigned lp_color; int lp_h, lp_w;
    int B, H, W, thickness, K;
    int* table; float* vertices; float* matrices; unsigned char* lp_valid;
};

// vertices -> the slot: truncation toward zero; a non-finite vertex or one beyond 2^20 disables the slot (its vertices read 0)
__device__ __forceinline__ void overlay_write_slot(int* __restrict__ slot, float* __restrict__ fv, const double* vx, const double* vy,
                                                   const float* fx, const float* fy, unsigned colour, int thickness, bool enabled) {
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 4; ++e) ok = ok && fabs(vx[e]) <= (double)OV_MAX_COORD && fabs(vy[e]) <= (double)OV_MAX_COORD;   // (false for a NaN)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        slot[2 * e] = ok ? (int)vx[e] : 0;
        slot[2 * e + 1] = ok ? (int)vy[e] : 0;
        if (fv) {
            fv[2 * e] = fx[e];
            fv[2 * e + 1] = fy[e];
        }
    }
    slot[8] = (int)colour;
    slot[9] = thickness;
    slot[10] = (enabled && ok) ? 1 : 0;
    slot[11] = 0;
}

// the 8 x 8 system of render.homography(LP_corner, corner_pts): unknowns m0..m7 of u = (m0 x + m1 y + m2) / (m6 x + m7 y + 1),
// v = (m3 x + m4 y + m5) / (m6 x + m7 y + 1).  Rows 0..3: [x, y, 1, 0, 0, 0, -x u, -y u | u], rows 4..7: [0, 0, 0, x, y, 1, -x v, -y v | v].
__device__ bool overlay_solve(const double* x, const double* y, const double* u, const double* v, double* m) {
    double A[8][9];
    for (int i = 0; i < 4; ++i) {
        A[i][0] = x[i]; A[i][1] = y[i]; A[i][2] = 1.0; A[i][3] = 0.0; A[i][4] = 0.0; A[i][5] = 0.0;
        A[i][6] = -x[i] * u[i]; A[i][7] = -y[i] * u[i]; A[i][8] = u[i];
        A[i + 4][0] = 0.0; A[i + 4][1] = 0.0; A[i + 4][2] = 0.0; A[i + 4][3] = x[i]; A[i + 4][4] = y[i]; A[i + 4][5] = 1.0;
        A[i + 4][6] = -x[i] * v[i]; A[i + 4][7] = -y[i] * v[i]; A[i + 4][8] = v[i];
    }
    bool ok = true;
    for (int k = 0; k < 8; ++k) {
        int p = k;
        double best = fabs(A[k][k]);
        for (int r = k + 1; r < 8; ++r) {
            const double a = fabs(A[r][k]);
            if (a > best) { best = a; p = r; }                 // strictly larger: the lowest row among equals (a NaN never wins)
        }
        if (p != k)
            for (int c = 0; c < 9; ++c) { const double t = A[k][c]; A[k][c] = A[p][c]; A[p][c] = t; }
        const double piv = A[k][k];
        if (!(fabs(piv) > 0.0) || !(fabs(piv) <= 1.7976931348623157e308)) { ok = false; break; }
        for (int r = k + 1; r < 8; ++r) {
            const double f = A[r][k] / piv;
            for (int c = k; c < 9; ++c) A[r][c] = A[r][c] - f * A[k][c];
        }
    }
    if (!ok) return false;
    for (int k = 7; k >= 0; --k) {
        double s = A[k][8];
        for (int c = k + 1; c < 8; ++c) s = s - A[k][c] * m[c];
        m[k] = s / A[k][k];
    }
    for (int k = 0; k < 8; ++k) ok = ok && fabs(m[k]) <= 1.7976931348623157e308;
    return ok;
}

__global__ __launch_bounds__(OV_SHAPE_THREADS) void overlay_shapes_kernel(OverlayShapesArgs a) {
    const int q = blockIdx.x * OV_SHAPE_THREADS + threadIdx.x;
    if (q >= a.B * a.K) return;
    const int b = q / a.K, s = q - b * a.K;
    int* slot = a.table + (long long)q * OV_SLOT_WORDS;
    float* fv = a.vertices ? a.vertices + (long long)q * 8 : nullptr;
    const int n_nms = a.rows ? a.post_nms : 0;
    const int s_pred = a.pred ? n_nms : -1;
    const double W = (double)a.W, H = (double)a.H;
    double vx[4], vy[4];
    float fx[4], fy[4];
    if (s < n_nms) {
        // kept position s: the box of candidate id = box * cand_per_box + class, [l, t, r, b] fractions of the frame, no rotation
        int cnt = a.kept_count[b];
        cnt = cnt < a.post_nms ? cnt : a.post_nms;
        const int id = s < cnt ? a.kept[(long long)b * a.post_nms + s] : -1;
        const int box = id >= 0 ? id / a.cand_per_box : -1;
        const bool have = box >= 0 && box < a.nbox;
        double l = 0.0, t = 0.0, r = 0.0, bo = 0.0;
        unsigned colour = 0;
        if (have) {
            const float* row = a.rows + ((long long)b * a.nbox + box) * a.rows_C;
            l = (double)row[1] * W; t = (double)row[2] * H; r = (double)row[3] * W; bo = (double)row[4] * H;
            const unsigned char* c = a.palette + 4 * ((id % a.cand_per_box) % a.npalette);
            colour = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16) | ((unsigned)c[3] << 24);
        }
        vx[0] = l; vy[0] = t; vx[1] = r; vy[1] = t; vx[2] = r; vy[2] = bo; vx[3] = l; vy[3] = bo;
#pragma unroll
        for (int e = 0; e < 4; ++e) { fx[e] = (float)vx[e]; fy[e] = (float)vy[e]; }
        overlay_write_slot(slot, fv, vx, vy, fx, fy, colour, a.thickness, have);
    } else if (s == s_pred) {
        // cv2_add_bbox (yolo_cv.py:253-266): b = [score, y, x, h, w, rot, ...]
        const float* p = a.pred + (long long)b * a.pred_C;
        const double r = a.use_r ? -(double)p[5] : 0.0;
        const double h = (double)p[3] * H, w = (double)p[4] * W;
        const double cr = cos(r), sr = sin(r);
        const double wc = (w * cr) / 2.0, hs = (h * sr) / 2.0, ws = (w * sr) / 2.0, hc = (h * cr) / 2.0;
        const double sx = (double)p[2] * W, sy = (double)p[1] * H;
        vx[0] = (wc - hs) + sx;   vy[0] = (ws + hc) + sy;
        vx[1] = (-wc - hs) + sx;  vy[1] = (-ws + hc) + sy;
        vx[2] = (-wc + hs) + sx;  vy[2] = (-ws - hc) + sy;
        vx[3] = (wc + hs) + sx;   vy[3] = (ws - hc) + sy;
#pragma unroll
        for (int e = 0; e < 4; ++e) { fx[e] = (float)vx[e]; fy[e] = (float)vy[e]; }
        overlay_write_slot(slot, fv, vx, vy, fx, fy, a.car_color, a.thickness, p[0] > a.car_threshold);
    } else {
        // ProjectRectangle6D.projection_matrix (:352-377) + __call__'s divide and float32 (:344-348) + add_edges' scaling (:382-386)
        const float* p = a.lp + (long long)b * 7;
        const double X = (double)p[1], Y = (double)p[2], Z = (double)p[3], r1 = (double)p[4], r2 = (double)p[5], r3 = (double)p[6];
        const double s1 = sin(r1), c1 = cos(r1), s2 = sin(r2), c2 = cos(r2), s3 = sin(r3), c3 = cos(r3);
        const double ta = s1 * c2 * 84.0, tb = s1 * s2 * c3 * 84.0, tc = s2 * 199.5, td = s3 * c1 * 84.0;
        const double te = c2 * c3 * 199.5, tf = s1 * s2 * s3 * 84.0, tg = s3 * c2 * 199.5, th = c1 * c3 * 84.0;
        double wz[4], nx[4], ny[4];
        wz[0] = Z + ta - tc;  wz[1] = Z + ta + tc;  wz[2] = Z - ta + tc;  wz[3] = Z - ta - tc;
        nx[0] = a.cx * wz[0] + a.fx * (X + tb - td + te);
        nx[1] = a.cx * wz[1] + a.fx * (X + tb - td - te);
        nx[2] = a.cx * wz[2] + a.fx * (X - tb + td - te);
        nx[3] = a.cx * wz[3] + a.fx * (X - tb + td + te);
        ny[0] = a.cy * wz[0] + a.fy * (Y + tf + tg + th);
        ny[1] = a.cy * wz[1] + a.fy * (Y + tf - tg + th);
        ny[2] = a.cy * wz[2] + a.fy * (Y - tf - tg - th);
        ny[3] = a.cy * wz[3] + a.fy * (Y - tf + tg - th);
        const float xs = (float)((double)a.W / (double)a.cam_w), ys = (float)((double)a.H / (double)a.cam_h);
        bool divides = true;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            divides = divides && wz[e] != 0.0;                  // (a NaN w passes here and fails the finite test of the vertices)
            fx[e] = (float)(nx[e] / wz[e]) * xs;
            fy[e] = (float)(ny[e] / wz[e]) * ys;
            vx[e] = (double)fx[e];
            vy[e] = (double)fy[e];
        }
        const bool wanted = p[0] > a.lp_threshold;
        overlay_write_slot(slot, fv, vx, vy, fx, fy, a.lp_color, a.thickness, wanted);
        // the plate image's corners in the reference's order (:392-395): bottom-right, bottom-left, top-left, top-right
        const double lw = (double)a.lp_w, lh = (double)a.lp_h;
        const double px[4] = {lw, 0.0, 0.0, lw}, py[4] = {lh, lh, 0.0, 0.0};
        double m[8];
        bool finite = true;
#pragma unroll
        for (int e = 0; e < 4; ++e) finite = finite && fabs(vx[e]) <= 1.7976931348623157e308 && fabs(vy[e]) <= 1.7976931348623157e308;
        bool valid = wanted && divides && finite;
        if (valid) valid = overlay_solve(px, py, vx, vy, m);
        float* M = a.matrices + (long long)b * 9;
        if (valid) {
#pragma unroll
            for (int k = 0; k < 8; ++k) M[k] = (float)m[k];
            M[8] = 1.f;
        } else {
            M[0] = 0.f; M[1] = 0.f; M[2] = -4.f; M[3] = 0.f; M[4] = 0.f; M[5] = -4.f; M[6] = 0.f; M[7] = 0.f; M[8] = 1.f;
        }
        a.lp_valid[b] = valid ? 1 : 0;
    }
}

extern "C" long long yolo_overlay_table_bytes(int B, int K) {
    if (B <= 0 || K <= 0) return YOLO_EINVAL;
    if (K > OV_MAX_K) return YOLO_EUNSUPPORTED;
    return (long long)B * K * OV_SLOT_WORDS * 4;
}

extern "C" int yolo_overlay_shapes(const float* rows, const int* kept, const int* kept_count, int nbox, int rows_C, int post_nms,
                                   int cand_per_box, const unsigned char* palette, int npalette, const float* pred, int pred_C,
                                   float car_threshold, int use_r, unsigned car_color, const float* lp, double fx, double fy,
                                   double cx, double cy, int cam_w, int cam_h, float lp_threshold, unsigned lp_color, int lp_h,
                                   int lp_w, int B, int H, int W, int thickness, int* table, int K, float* vertices,
                                   float* matrices, unsigned char* lp_valid, void* stream) {
    if (!table || B <= 0 || H <= 0 || W <= 0 || K <= 0 || thickness <= 0) return YOLO_EINVAL;
    if (!rows && !pred && !lp) return YOLO_EINVAL;
    if (rows && (!kept || !kept_count || !palette || nbox <= 0 || rows_C < 5 || post_nms <= 0 || cand_per_box <= 0 || npalette <= 0))
        return YOLO_EINVAL;
    if (pred && pred_C < 6) return YOLO_EINVAL;
    if (lp && (!matrices || !lp_valid || cam_w <= 0 || cam_h <= 0 || lp_h <= 0 || lp_w <= 0)) return YOLO_EINVAL;
    if (K != (rows ? post_nms : 0) + (pred ? 1 : 0) + (lp ? 1 : 0)) return YOLO_EINVAL;
    if ((reinterpret_cast<unsigned long long>(table) & 15ull) || (reinterpret_cast<unsigned long long>(vertices) & 3ull) ||
        (reinterpret_cast<unsigned long long>(matrices) & 3ull))
        return YOLO_EINVAL;
    if (K > OV_MAX_K || H > OV_MAX_SIDE || W > OV_MAX_SIDE || thickness > OV_MAX_T) return YOLO_EUNSUPPORTED;
    if ((long long)B * K > 0x7fffff00LL) return YOLO_EUNSUPPORTED;
    OverlayShapesArgs a;
    a.rows = rows; a.kept = kept; a.kept_count = kept_count; a.nbox = nbox; a.rows_C = rows_C; a.post_nms = post_nms;
    a.cand_per_box = cand_per_box; a.palette = palette; a.npalette = npalette;
    a.pred = pred; a.pred_C = pred_C; a.car_threshold = car_threshold; a.use_r = use_r; a.car_color = car_color;
    a.lp = lp; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.cam_w = cam_w; a.cam_h = cam_h; a.lp_threshold = lp_threshold;
    a.lp_color = lp_color; a.lp_h = lp_h; a.lp_w = lp_w;
    a.B = B; a.H = H; a.W = W; a.thickness = thickness; a.K = K;
    a.table = table; a.vertices = vertices; a.matrices = matrices; a.lp_valid = lp_valid;
    const unsigned grid = (unsigned)(((long long)B * K + OV_SHAPE_THREADS - 1) / OV_SHAPE_THREADS);
    YOLO_LAUNCH(overlay_shapes_kernel, dim3(grid), dim3(OV_SHAPE_THREADS), 0, (hipStream_t)stream, a);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// ---- draw -----------------------------------------------------------------------------------------------------------------------

struct OverlaySeg {
    int ax, ay, dx, dy;                                  // A and d = B - A
    int bx0, by0, bx1, by1;                              // the segment's bounding box grown by ceil(t / 2), inclusive
    long long dd;                                        // d . d
    int t2;                                              // t * t
    unsigned colour;
};

// 4 dist^2 <= t^2 in integers (the header's three cases); every product stays inside 64 bits for |A|, |B| <= 2^20, 0 <= P < 2^14
__device__ __forceinline__ bool overlay_hit(const OverlaySeg& g, int x, int y) {
    if (x < g.bx0 || x > g.bx1 || y < g.by0 || y > g.by1) return false;      // (farther than t / 2 from the whole segment)
    const long long px = (long long)x - g.ax, py = (long long)y - g.ay;
    const long long dx = g.dx, dy = g.dy;
    const long long u = px * dx + py * dy;
    const long long t2 = g.t2;
    if (u <= 0) return 4 * (px * px + py * py) <= t2;
    if (u >= g.dd) {
        const long long qx = px - dx, qy = py - dy;
        return 4 * (qx * qx + qy * qy) <= t2;
    }
    long long cr = px * dy - py * dx;
    cr = cr < 0 ? -cr : cr;
    if (cr >= (1LL << 31)) return false;                 // 4 cr^2 >= 2^64 > t^2 (d.d)
    const unsigned long long c = (unsigned long long)cr;
    return 4ull * (c * c) <= (unsigned long long)t2 * (unsigned long long)g.dd;
}

// grid (tiles_x * tiles_y, images); thread t: wave t / 64 owns rows 8 (t / 64)..+7 of the tile, lane l columns 4 l..4 l + 3
template <int C>
__global__ __launch_bounds__(OV_THREADS) void overlay_draw_kernel(unsigned char* __restrict__ frames, const int* __restrict__ table,
                                                                  int H, int W, int K, int tiles_x) {
    __shared__ OverlaySeg seg[OV_MAX_SEG];
    __shared__ unsigned char meets[OV_MAX_SEG];
    __shared__ unsigned short list[OV_MAX_SEG];
    __shared__ int n_list;
    const int tid = threadIdx.x;
    const long long n = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x_lo = tx * OV_TILE_W, y_lo = ty * OV_TILE_H;
    const int x_hi = min(x_lo + OV_TILE_W, W) - 1, y_hi = min(y_lo + OV_TILE_H, H) - 1;
    const int* tab = table + n * K * OV_SLOT_WORDS;
    const int nseg = K * 4;
    for (int g = tid; g < nseg; g += OV_THREADS) {
        const int s = g >> 2, e = g & 3;
        // the slot's 12 words as three 16-byte loads issued together (the table is 16-byte aligned and a slot is 48 bytes)
        const int4* slot4 = reinterpret_cast<const int4*>(tab + s * OV_SLOT_WORDS);
        const int4 q0 = slot4[0], q1 = slot4[1], q2 = slot4[2];
        const int v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        const int t = q2.y;
        bool on = (q2.z != 0) & (t >= 1) & (t <= OV_MAX_T);
#pragma unroll
        for (int k = 0; k < 8; ++k) on = on & (v[k] >= -OV_MAX_COORD) & (v[k] <= OV_MAX_COORD);
        const int ax = e == 0 ? v[0] : e == 1 ? v[2] : e == 2 ? v[4] : v[6], ay = e == 0 ? v[1] : e == 1 ? v[3] : e == 2 ? v[5] : v[7];
        const int bx = e == 0 ? v[2] : e == 1 ? v[4] : e == 2 ? v[6] : v[0], by = e == 0 ? v[3] : e == 1 ? v[5] : e == 2 ? v[7] : v[1];
        const int grow = (t + 1) >> 1;
        OverlaySeg sg;
        sg.ax = ax; sg.ay = ay; sg.dx = bx - ax; sg.dy = by - ay;
        sg.bx0 = min(ax, bx) - grow; sg.bx1 = max(ax, bx) + grow; sg.by0 = min(ay, by) - grow; sg.by1 = max(ay, by) + grow;
        sg.dd = (long long)sg.dx * sg.dx + (long long)sg.dy * sg.dy;
        sg.t2 = t * t;
        sg.colour = (unsigned)q2.x;
        on = on && sg.bx0 <= x_hi && sg.bx1 >= x_lo && sg.by0 <= y_hi && sg.by1 >= y_lo;
        if (on) seg[g] = sg;
        meets[g] = on ? 1 : 0;
    }
    __syncthreads();
    if (tid < 64) {                                      // wave 0: the segments that meet the tile, in slot order
        int base = 0;
        for (int g0 = 0; g0 < nseg; g0 += 64) {
            const int g = g0 + tid;
            const bool on = g < nseg && meets[g] != 0;
            const unsigned long long mask = __ballot(on);
            if (on) list[base + __popcll(mask & ((1ull << tid) - 1ull))] = (unsigned short)g;
            base += __popcll(mask);
        }
        if (tid == 0) n_list = base;
    }
    __syncthreads();
    const int count = n_list;
    if (count == 0) return;
    // a wave owns whole rows: a segment whose grown box misses the row is skipped by the whole wave, one that misses the lane's run
    // of OV_RUN pixels by the lane; only what is left meets the exact test.  From the highest slot down, so the first hit is final.
    const int x0 = x_lo + (tid & 63) * OV_RUN;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned char* img = frames + n * H * W * C;
    unsigned outside = 0;                                // the pixels of the run beyond the frame's last column
#pragma unroll
    for (int e = 0; e < OV_RUN; ++e) outside |= (x0 + e > x_hi) ? (1u << e) : 0u;
    for (int r = 0; r < OV_WAVE_ROWS; ++r) {
        const int y = y_lo + wave * OV_WAVE_ROWS + r;
        if (y > y_hi) break;
        unsigned done = outside;
        unsigned col[OV_RUN];
        for (int k = count - 1; k >= 0 && done != (1u << OV_RUN) - 1u; --k) {
            const OverlaySeg& g = seg[list[k]];
            if (y < g.by0 || y > g.by1) continue;
            if (x0 + OV_RUN - 1 < g.bx0 || x0 > g.bx1) continue;
#pragma unroll
            for (int e = 0; e < OV_RUN; ++e) {
                if (!((done >> e) & 1u) && overlay_hit(g, x0 + e, y)) {
                    done |= 1u << e;
                    col[e] = g.colour;
                }
            }
        }
        done &= ~outside;
        if (done == 0) continue;
        unsigned char* p = img + ((long long)y * W + x0) * C;
#pragma unroll
        for (int e = 0; e < OV_RUN; ++e) {
            if ((done >> e) & 1u) {
#pragma unroll
                for (int c = 0; c < C; ++c) p[e * C + c] = (unsigned char)(col[e] >> (8 * c));
            }
        }
    }
}

template <int C>
static int overlay_draw_launch(unsigned char* frames, const int* table, int N, int H, int W, int K, hipStream_t stream) {
    const int tiles_x = (W + OV_TILE_W - 1) / OV_TILE_W, tiles_y = (H + OV_TILE_H - 1) / OV_TILE_H;
    const long long img = (long long)H * W * C;
    for (int n0 = 0; n0 < N; n0 += 65535) {              // (grid.y holds at most 65535 images)
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        YOLO_LAUNCH((overlay_draw_kernel<C>), dim3(tiles_x * tiles_y, nb), dim3(OV_THREADS), 0, stream, frames + n0 * img,
                    table + (long long)n0 * K * OV_SLOT_WORDS, H, W, K, tiles_x);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

extern "C" int yolo_overlay_draw(unsigned char* frames, const int* table, int N, int H, int W, int C, int K, void* stream) {
    if (!frames || !table) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0) return YOLO_EINVAL;
    if (reinterpret_cast<unsigned long long>(table) & 15ull) return YOLO_EINVAL;
    if (K > OV_MAX_K || C > OV_MAX_C || H > OV_MAX_SIDE || W > OV_MAX_SIDE) return YOLO_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: return overlay_draw_launch<1>(frames, table, N, H, W, K, s);
        case 2: return overlay_draw_launch<2>(frames, table, N, H, W, K, s);
        case 3: return overlay_draw_launch<3>(frames, table, N, H, W, K, s);
        default: return overlay_draw_launch<4>(frames, table, N, H, W, K, s);
    }
}

// ---- labels ---------------------------------------------------------------------------------------------------------------------

constexpr int OV_LABEL_WORDS = YOLO_OVERLAY_LABEL_WORDS;  // x y text-colour ground-colour flags nchar text[10]
constexpr int OV_LABEL_CHARS = YOLO_OVERLAY_LABEL_CHARS;
constexpr int OV_NAME_BYTES = YOLO_OVERLAY_NAME_BYTES;
constexpr int OV_MAX_CELL = 32;
constexpr int OV_MAX_SCALE = 16;
constexpr long long OV_LABEL_SAT = 1LL << 30;             // x and y are made in 64 bits and saturated to +-2^30 (the raster refuses beyond 2^20)

struct OverlayLabelsArgs {
    const int* table;
    const float* rows; const int* kept; const int* kept_count; const float* kept_scores; int nbox, rows_C, post_nms, cand_per_box;
    const float* pred; int pred_C; const float* pose; int show_deg;
    const float* lp;
    const unsigned char* names; int nname;
    int cell_w, cell_h, advance, scale, gap, pad, ground; unsigned ground_colour;
    int B, H, W, K;
    int* labels;
};

__device__ __forceinline__ int overlay_put(unsigned* text, int n, unsigned ch) {
    text[n >> 2] |= (ch & 255u) << (8 * (n & 3));
    return n + 1;
}

// [name ' '] score [' ' deg] -> text bytes, returns nchar (at most 16 + 1 + 5 + 1 + 4 = 27)
__device__ int overlay_compose(unsigned* text, const unsigned char* name, float score, bool have_deg, float azimuth) {
    int n = 0;
    if (name && name[0] != 0) {
        for (int i = 0; i < OV_NAME_BYTES && name[i] != 0; ++i) n = overlay_put(text, n, name[i]);
        n = overlay_put(text, n, ' ');
    }
    if (score >= 0.f && score <= FLT_MAX) {
        // (double)score * 1000.0 is exact (24 x 10 significant bits): the nearest integer, ties to even, is '%.3f' digit for digit
        const double d = (double)score * 1000.0;
        const int v = d >= 9999.0 ? 9999 : (int)llrint(d);
        n = overlay_put(text, n, '0' + v / 1000);
        n = overlay_put(text, n, '.');
        n = overlay_put(text, n, '0' + (v / 100) % 10);
        n = overlay_put(text, n, '0' + (v / 10) % 10);
        n = overlay_put(text, n, '0' + v % 10);
    } else {
        n = overlay_put(text, n, '-');
        n = overlay_put(text, n, '.');
        for (int i = 0; i < 3; ++i) n = overlay_put(text, n, '-');
    }
    if (have_deg && fabsf(azimuth) <= FLT_MAX) {
        const double d = rint((double)azimuth * 57.29577951308232);
        if (fabs(d) <= 999.0) {
            int v = (int)d;
            n = overlay_put(text, n, ' ');
            if (v < 0) { n = overlay_put(text, n, '-'); v = -v; }
            if (v >= 100) n = overlay_put(text, n, '0' + v / 100);
            if (v >= 10) n = overlay_put(text, n, '0' + (v / 10) % 10);
            n = overlay_put(text, n, '0' + v % 10);
        }
    }
    return n;
}

__device__ __forceinline__ int overlay_sat(long long v) {
    return (int)(v < -OV_LABEL_SAT ? -OV_LABEL_SAT : v > OV_LABEL_SAT ? OV_LABEL_SAT : v);
}

__global__ __launch_bounds__(OV_SHAPE_THREADS) void overlay_labels_kernel(OverlayLabelsArgs a) {
    const int q = blockIdx.x * OV_SHAPE_THREADS + threadIdx.x;
    if (q >= a.B * a.K) return;
    const int b = q / a.K, s = q - b * a.K;
    const int4* slot4 = reinterpret_cast<const int4*>(a.table + (long long)q * OV_SLOT_WORDS);
    const int4 q0 = slot4[0], q1 = slot4[1], q2 = slot4[2];
    const int n_nms = a.rows ? a.post_nms : 0;
    const int s_pred = a.pred ? n_nms : -1;
    bool on = q2.z != 0;
    float score = 0.f, azimuth = 0.f;
    int cls = -1;
    bool have_deg = false;
    if (s < n_nms) {
        // the id test of overlay_shapes_kernel again: no row is read through an id it refused
        int cnt = a.kept_count[b];
        cnt = cnt < a.post_nms ? cnt : a.post_nms;
        const int id = s < cnt ? a.kept[(long long)b * a.post_nms + s] : -1;
        const int box = id >= 0 ? id / a.cand_per_box : -1;
        on = on && box >= 0 && box < a.nbox;
        if (on) {
            cls = a.cand_per_box > 1 ? id % a.cand_per_box : -1;
            score = a.kept_scores ? a.kept_scores[(long long)b * a.post_nms + s] : a.rows[((long long)b * a.nbox + box) * a.rows_C];
        }
    } else if (s == s_pred) {
        score = a.pred[(long long)b * a.pred_C];
        if (a.pose) {
            const float4 po = reinterpret_cast<const float4*>(a.pose)[b];
            if (po.w > -1.f && po.w < (float)a.nname) cls = (int)po.w;      // (false for a NaN)
            have_deg = a.show_deg != 0;
            azimuth = po.x;
        }
    } else {
        score = a.lp[(long long)b * 7];
    }
    unsigned text[OV_LABEL_CHARS / 4];
#pragma unroll
    for (int i = 0; i < OV_LABEL_CHARS / 4; ++i) text[i] = 0u;
    int nchar = 0, x = 0, y = 0;
    if (on) {
        const unsigned char* name = (cls >= 0 && cls < a.nname) ? a.names + (long long)cls * OV_NAME_BYTES : nullptr;
        nchar = overlay_compose(text, name, score, have_deg, azimuth);
        const long long bx0 = min(min(q0.x, q0.z), min(q1.x, q1.z)), by0 = min(min(q0.y, q0.w), min(q1.y, q1.w));
        const long long Th = (long long)a.cell_h * a.scale, Tw = ((long long)(nchar - 1) * a.advance + a.cell_w) * a.scale;
        long long ly = by0 - a.gap - Th;
        if (ly - a.pad < 0) ly = by0 + a.gap;                            // no room above: under the box's top edge
        long long lx = bx0;
        if (lx + Tw + a.pad > a.W) lx = (long long)a.W - Tw - a.pad;
        if (lx - a.pad < 0) lx = a.pad;
        x = overlay_sat(lx);
        y = overlay_sat(ly);
    }
    int4* out = reinterpret_cast<int4*>(a.labels + (long long)q * OV_LABEL_WORDS);
    out[0] = make_int4(x, y, on ? q2.x : 0, on ? (int)a.ground_colour : 0);
    out[1] = make_int4(on ? (1 | (a.ground ? 2 : 0)) : 0, nchar, (int)text[0], (int)text[1]);
    out[2] = make_int4((int)text[2], (int)text[3], (int)text[4], (int)text[5]);
    out[3] = make_int4((int)text[6], (int)text[7], (int)text[8], (int)text[9]);
}

extern "C" int yolo_overlay_labels(const int* table, const float* rows, const int* kept, const int* kept_count, const float* kept_scores,
                                   int nbox, int rows_C, int post_nms, int cand_per_box, const float* pred, int pred_C,
                                   const float* pose, int show_deg, const float* lp, const unsigned char* names, int nname, int cell_w,
                                   int cell_h, int advance, int scale, int gap, int pad, int ground, unsigned ground_colour, int B,
                                   int H, int W, int K, int* labels, void* stream) {
    if (!table || !labels || B <= 0 || H <= 0 || W <= 0 || K <= 0) return YOLO_EINVAL;
    if (!rows && !pred && !lp) return YOLO_EINVAL;
    if (rows && (!kept || !kept_count || nbox <= 0 || rows_C < 5 || post_nms <= 0 || cand_per_box <= 0)) return YOLO_EINVAL;
    if (pred && pred_C < 6) return YOLO_EINVAL;
    if (K != (rows ? post_nms : 0) + (pred ? 1 : 0) + (lp ? 1 : 0)) return YOLO_EINVAL;
    if (nname < 0 || (nname > 0 && !names)) return YOLO_EINVAL;
    if (cell_w < 1 || cell_h < 1 || scale < 1 || advance < cell_w || gap < 0 || pad < 0) return YOLO_EINVAL;
    if (ground != 0 && ground != 1) return YOLO_EINVAL;
    if ((reinterpret_cast<unsigned long long>(table) & 15ull) || (reinterpret_cast<unsigned long long>(labels) & 15ull) ||
        (reinterpret_cast<unsigned long long>(pose) & 15ull))
        return YOLO_EINVAL;
    if (K > OV_MAX_K || cell_w > OV_MAX_CELL || cell_h > OV_MAX_CELL || scale > OV_MAX_SCALE || H > OV_MAX_SIDE || W > OV_MAX_SIDE)
        return YOLO_EUNSUPPORTED;
    if ((long long)B * K > 0x7fffff00LL) return YOLO_EUNSUPPORTED;
    OverlayLabelsArgs a;
    a.table = table;
    a.rows = rows; a.kept = kept; a.kept_count = kept_count; a.kept_scores = kept_scores; a.nbox = nbox; a.rows_C = rows_C;
    a.post_nms = post_nms; a.cand_per_box = cand_per_box;
    a.pred = pred; a.pred_C = pred_C; a.pose = pose; a.show_deg = show_deg; a.lp = lp; a.names = names; a.nname = nname;
    a.cell_w = cell_w; a.cell_h = cell_h; a.advance = advance; a.scale = scale; a.gap = gap; a.pad = pad; a.ground = ground;
    a.ground_colour = ground_colour;
    a.B = B; a.H = H; a.W = W; a.K = K; a.labels = labels;
    const unsigned grid = (unsigned)(((long long)B * K + OV_SHAPE_THREADS - 1) / OV_SHAPE_THREADS);
    YOLO_LAUNCH(overlay_labels_kernel, dim3(grid), dim3(OV_SHAPE_THREADS), 0, (hipStream_t)stream, a);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// ---- text -----------------------------------------------------------------------------------------------------------------------
// The grid follows the labels, not the frame: block (tile, k, image) owns one OV_TEXT_TILE_W x OV_TEXT_TILE_H tile of label k's
// paint rectangle (its ground box, or its text box without a ground) clipped to the frame; the grid holds as many tiles as the
// largest label these metrics allow, and a block whose tile lies beyond its label's rectangle, or whose label is disabled or empty,
// leaves at once.  The block keeps the font rows of the label's characters in LDS (row r of character i at [i cell_h + r]; a byte
// outside the font: zeros), and the paint rectangles of the enabled labels ABOVE k that meet the tile (wave 0 compacts them: ballot
// + popcount, no atomics).  A thread owns one column of the tile -- its character, glyph column and ground membership are fixed --
// and walks the rows; a pixel is stored iff label k paints it and no label above does, so every pixel has one writer whatever the
// block order.  Byte stores, no frame byte read.

constexpr int OV_TEXT_THREADS = 256;
constexpr int OV_TEXT_TILE_W = OV_TEXT_THREADS;         // one column per thread
constexpr int OV_TEXT_TILE_H = 16;
constexpr int OV_TEXT_CLAMP = 1 << 22;                  // an advance x scale or a pad beyond this acts like this inside any frame

struct OverlayTextArgs {
    int nglyph, first_code, cell_h, scale, step, pad, cw_px, th;      // step = advance x scale, cw_px = cell_w x scale, th = cell_h x scale
    int H, W, K, tiles_x;
};

struct OverlayTextRect {
    int x0, y0, x1, y1;                                  // the pixels a label may paint, [x0, x1) x [y0, y1), not clipped
    int x, y, nchar, ground;
};

// words 0..7 of a label -> its paint rectangle; false: not enabled, or no character (such a label paints nothing)
__device__ __forceinline__ bool overlay_text_rect(const int4 q0, const int4 q1, const OverlayTextArgs& a, OverlayTextRect& r) {
    const int x = q0.x, y = q0.y, flags = q1.x, nchar = q1.y;
    if (!(flags & 1) || nchar < 1 || nchar > OV_LABEL_CHARS) return false;
    if (x < -OV_MAX_COORD || x > OV_MAX_COORD || y < -OV_MAX_COORD || y > OV_MAX_COORD) return false;
    const int tw = (nchar - 1) * a.step + a.cw_px;       // < 39 x 2^22 + 2^9
    const int grow = (flags & 2) ? a.pad : 0;
    r.x0 = x - grow; r.x1 = x + tw + grow; r.y0 = y - grow; r.y1 = y + a.th + grow;
    r.x = x; r.y = y; r.nchar = nchar; r.ground = (flags & 2) ? 1 : 0;
    return true;
}

// is (px, py), a pixel inside the label's text box, ink?  The label's text and the font come from global memory: this is the path of
// a label ABOVE the block's own that has no ground box.
__device__ bool overlay_text_ink(const int* __restrict__ lab, const unsigned* __restrict__ font, const OverlayTextArgs& a, int px, int py) {
    const int rx = px - lab[0], ty = py - lab[1];
    const int i = rx / a.step, cx = rx - i * a.step;
    if (cx >= a.cw_px) return false;
    const long long g = (long long)(((unsigned)lab[6 + (i >> 2)] >> (8 * (i & 3))) & 255u) - a.first_code;
    if (g < 0 || g >= a.nglyph) return false;
    return (font[g * a.cell_h + ty / a.scale] >> (cx / a.scale)) & 1u;
}

template <int C>
__global__ __launch_bounds__(OV_TEXT_THREADS) void overlay_text_kernel(unsigned char* __restrict__ frames, const int* __restrict__ labels,
                                                                       const unsigned* __restrict__ font, OverlayTextArgs a) {
    __shared__ unsigned glyph[OV_LABEL_CHARS * OV_MAX_CELL];
    __shared__ OverlayTextRect cand[OV_MAX_K];
    __shared__ unsigned char meets[OV_MAX_K];
    __shared__ unsigned char list[OV_MAX_K];             // positions in cand[] of the labels above that meet the tile
    __shared__ int n_list;
    const int tid = threadIdx.x;
    const int k = blockIdx.y;
    const long long n = blockIdx.z;
    const int* img_labels = labels + n * a.K * OV_LABEL_WORDS;
    const int* lab = img_labels + k * OV_LABEL_WORDS;
    const int4* lab4 = reinterpret_cast<const int4*>(lab);
    const int4 q0 = lab4[0], q1 = lab4[1];
    OverlayTextRect own;
    if (!overlay_text_rect(q0, q1, a, own)) return;      // (the same for every thread of the block, as every return before the barriers)
    const int cx0 = max(own.x0, 0), cy0 = max(own.y0, 0), cx1 = min(own.x1, a.W), cy1 = min(own.y1, a.H);
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    // (cx0 <= 2^20 + 2^22 and tx < 64: no overflow)
    const int x_lo = cx0 + tx * OV_TEXT_TILE_W, y_lo = cy0 + ty * OV_TEXT_TILE_H;
    if (x_lo >= cx1 || y_lo >= cy1) return;
    const int x_hi = min(x_lo + OV_TEXT_TILE_W, cx1), y_hi = min(y_lo + OV_TEXT_TILE_H, cy1);      // exclusive
    for (int e = tid; e < own.nchar * a.cell_h; e += OV_TEXT_THREADS) {
        const int i = e / a.cell_h, r = e - i * a.cell_h;
        const long long g = (long long)(((unsigned)lab[6 + (i >> 2)] >> (8 * (i & 3))) & 255u) - a.first_code;
        glyph[e] = (g >= 0 && g < a.nglyph) ? font[g * a.cell_h + r] : 0u;
    }
    const int n_above = a.K - 1 - k;                     // <= 127: one pass
    if (tid < n_above) {
        const int4* h4 = reinterpret_cast<const int4*>(img_labels + (k + 1 + tid) * OV_LABEL_WORDS);
        OverlayTextRect r;
        bool on = overlay_text_rect(h4[0], h4[1], a, r);
        on = on && r.x0 < x_hi && r.x1 > x_lo && r.y0 < y_hi && r.y1 > y_lo;
        if (on) cand[tid] = r;
        meets[tid] = on ? 1 : 0;
    }
    __syncthreads();
    if (tid < 64) {
        int base = 0;
        for (int g0 = 0; g0 < n_above; g0 += 64) {
            const int g = g0 + tid;
            const bool on = g < n_above && meets[g] != 0;
            const unsigned long long mask = __ballot(on);
            if (on) list[base + __popcll(mask & ((1ull << tid) - 1ull))] = (unsigned char)g;
            base += __popcll(mask);
        }
        if (tid == 0) n_list = base;
    }
    __syncthreads();
    const int px = x_lo + tid;
    if (px >= x_hi) return;
    const int count = n_list;
    // the column's character and glyph column in the own label (ichar < 0: between two cells, or beside the text in the ground box)
    const int rx = px - own.x;
    int ichar = -1, col = 0;
    if (rx >= 0) {
        const int i = rx / a.step, cx = rx - i * a.step;
        if (i < own.nchar && cx < a.cw_px) { ichar = i; col = cx / a.scale; }
    }
    if (ichar < 0 && !own.ground) return;
    const unsigned ink_colour = (unsigned)q0.z, ground_colour = (unsigned)q0.w;
    unsigned char* img = frames + n * a.H * a.W * C;
    for (int py = y_lo; py < y_hi; ++py) {
        const int ry = py - own.y;
        bool ink = false;
        if (ichar >= 0 && ry >= 0 && ry < a.th) ink = (glyph[ichar * a.cell_h + ry / a.scale] >> col) & 1u;
        if (!ink && !own.ground) continue;
        bool covered = false;
        for (int e = 0; e < count && !covered; ++e) {
            const int h = list[e];
            const OverlayTextRect& r = cand[h];
            if (px < r.x0 || px >= r.x1 || py < r.y0 || py >= r.y1) continue;
            covered = r.ground ? true : overlay_text_ink(img_labels + (k + 1 + h) * OV_LABEL_WORDS, font, a, px, py);
        }
        if (covered) continue;
        const unsigned colour = ink ? ink_colour : ground_colour;
        unsigned char* p = img + ((long long)py * a.W + px) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = (unsigned char)(colour >> (8 * c));
    }
}

template <int C>
static int overlay_text_launch(unsigned char* frames, const int* labels, const unsigned* font, const OverlayTextArgs& a, int tiles,
                               int N, hipStream_t stream) {
    const long long img = (long long)a.H * a.W * C;
    for (int n0 = 0; n0 < N; n0 += 65535) {              // (grid.z holds at most 65535 images)
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        YOLO_LAUNCH((overlay_text_kernel<C>), dim3(tiles, a.K, nb), dim3(OV_TEXT_THREADS), 0, stream, frames + n0 * img,
                    labels + (long long)n0 * a.K * OV_LABEL_WORDS, font, a);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

extern "C" int yolo_overlay_text(unsigned char* frames, const int* labels, const unsigned* font, int nglyph, int first_code, int cell_w,
                                 int cell_h, int advance, int scale, int pad, int N, int H, int W, int C, int K, void* stream) {
    if (!frames || !labels || !font) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || nglyph <= 0 || cell_w <= 0 || cell_h <= 0 || scale <= 0) return YOLO_EINVAL;
    if (advance < cell_w || pad < 0) return YOLO_EINVAL;
    if ((reinterpret_cast<unsigned long long>(labels) & 15ull) || (reinterpret_cast<unsigned long long>(font) & 3ull)) return YOLO_EINVAL;
    if (K > OV_MAX_K || C > OV_MAX_C || H > OV_MAX_SIDE || W > OV_MAX_SIDE || cell_w > OV_MAX_CELL || cell_h > OV_MAX_CELL ||
        scale > OV_MAX_SCALE || nglyph > 256)
        return YOLO_EUNSUPPORTED;
    OverlayTextArgs a;
    a.nglyph = nglyph; a.first_code = first_code; a.cell_h = cell_h; a.scale = scale;
    // with |x| <= 2^20 and a frame of at most 2^14 pixels a side, a second cell 2^22 pixels on, or a ground box grown by 2^22, is where
    // any larger value would put it for every pixel of the frame
    const long long step = (long long)advance * scale;
    a.step = step > OV_TEXT_CLAMP ? OV_TEXT_CLAMP : (int)step;
    a.pad = pad > OV_TEXT_CLAMP ? OV_TEXT_CLAMP : pad;
    a.cw_px = cell_w * scale; a.th = cell_h * scale;
    a.H = H; a.W = W; a.K = K;
    const long long max_w = (long long)(OV_LABEL_CHARS - 1) * a.step + a.cw_px + 2LL * a.pad, max_h = (long long)a.th + 2LL * a.pad;
    const int span_w = (int)(max_w < W ? max_w : W), span_h = (int)(max_h < H ? max_h : H);
    a.tiles_x = (span_w + OV_TEXT_TILE_W - 1) / OV_TEXT_TILE_W;
    const int tiles = a.tiles_x * ((span_h + OV_TEXT_TILE_H - 1) / OV_TEXT_TILE_H);               // <= 64 x 1024
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: return overlay_text_launch<1>(frames, labels, font, a, tiles, N, s);
        case 2: return overlay_text_launch<2>(frames, labels, font, a, tiles, N, s);
        case 3: return overlay_text_launch<3>(frames, labels, font, a, tiles, N, s);
        default: return overlay_text_launch<4>(frames, labels, font, a, tiles, N, s);
    }
}
