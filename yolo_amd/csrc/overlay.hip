// The drawing end of the video node on the device for gfx950: the car box of cv2_add_bbox (yolo_modules/yolo_cv.py:239-270), the plate
// edges and the inverse map of the clipped plate of ProjectRectangle6D.add_edges (licence_plate_render/__init__.py:379-402), and the
// NMS boxes, from the rows where the detection kernels left them:
//   overlay_shapes_kernel   one thread per (image, slot): the slot's four integer vertices, colour, thickness and enabled flag; the
//                           plate's thread also solves the 8 x 8 system of the plate-image -> frame homography (fp64 Gaussian
//                           elimination with partial pivoting) and writes the (9) fp32 matrix yolo_warp_u8_to_nchw reads, and lp_valid
//   overlay_draw_kernel     one block per 256 x 32 pixel tile of one image: the image's 4 K segments go to LDS with their
//                           t/2-expanded bounding boxes, wave 0 compacts those that meet the tile (ballot + popcount: ordered, no
//                           atomics), and each thread tests its pixels against the list from the highest slot down -- the first hit is
//                           the colour.  The distance rule is exact integer arithmetic (include/yolo_amd.h, yolo_overlay_draw).
// Compiled with -ffp-contract=off: the shapes are the op-by-op fp64 / fp32 definition of the header, tests/overlay_ref.py restates it.
// The draw kernel reads no frame byte and stores only painted pixels (byte stores: the frame may start at any address); a tile no
// segment meets leaves after the compaction, so an image without an enabled shape is never addressed.
#include "common.h"

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
