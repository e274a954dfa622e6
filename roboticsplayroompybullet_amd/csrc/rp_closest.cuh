/* rp_closest.cuh - closest points between colliders (PyBullet's getClosestPoints) over the collider pose table of rp_render.cuh: live envs or stored state rows.
 *
 * The shapes are the ray caster's, without margins: a box collider is its exact box (R, p, he of its record), a sphere is centre and radius, a robot link with a hull
 * (RC_HULL) is the convex hull of its baked vertices, a robot link without one its box.  Any two colliders of one row may be asked.
 *
 * k_closest_points: one wave per row, as k_ray_test.  The wave stages the row's records in LDS and, one lane per collider, the BODY frame of every hull (hullv / hcv
 * are in the owning body's frame, the record is the collider's: body = record x inverse of the constant collider-to-body transform collider_xf applies, composed in
 * double and kept in fp32) and every collider's world AABB.  Then A LANE PER PAIR, pairs lane, lane + 64, ...: GJK's distance phase on the two support functions
 *   box     the sign of the direction per axis (direction rotated into the box's frame in fp32),
 *   sphere  its centre; the radius comes off the distance and moves the witness along the normal,
 *   hull    the scan of the direction's cell of the support-vertex candidate tables: direction rotated into the hull's frame in fp32, the largest computed coordinate
 *           wins, the lowest vertex number among equals (hcell_of; the rule tests/test_hull_cells.py holds),
 * with the Minkowski-difference points and the support point on A of every simplex vertex in DOUBLE, in registers; the sub-simplex step is gjk_seg / gjk_tri and the
 * tetrahedron rule of gjk_closest (the closest of the faces the origin lies outside of, the lowest face among equals; none: the origin is inside), its four faces one
 * after the other in the lane.  The stopping tests are the contact model's (GJK_DUP, GJK_REL, GJK_ZERO, GJK_STALL); the loop is bounded by RP_CP_ITERS support
 * queries, and a pair that reaches the bound reports the distance of its last simplex - an upper bound of the true one - with RP_CP_CAPPED set.
 * No atomics; every value a pair or a group gets depends on that row's records and the pair list alone, so a call gives the same bits on every run.
 *
 * Why a lane per pair and not a DPP row per pair: the wave's 64 pairs run side by side with the simplex in registers and no cross-lane traffic; the support queries
 * diverge by shape kind (three short paths) and by the cell's candidate count, the simplex step by its size.  A row per pair would spread one hull scan over 16 lanes
 * - a cell holds 3 - 8 candidates at the median - and leave 15 lanes idle through the double-precision simplex arithmetic, which is most of a round. */
#pragma once

static_assert((RP_MAX_COL & (RP_MAX_COL - 1)) == 0, "collider numbers are masked with RP_MAX_COL - 1");
#define RP_CP_ITERS 48
#define RP_CP_MAX_PAIRS 4096
#define RP_CP_MAX_GROUPS 64
#define CP_BOX 0
#define CP_SPHERE 1
#define CP_HULL 2

__device__ __forceinline__ D3 dadd(D3 a, D3 b) { return mkd(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ D3 dscale(D3 a, double s) { return mkd(a.x * s, a.y * s, a.z * s); }

/* the point of the shape farthest along d (world), in double from the fp32 record: rec = the collider's record, bf = its body frame (R9 p3; hulls only) */
__device__ __forceinline__ D3 cp_support(const DevModel* __restrict__ m, int kind, const float* rec, const float* bf, int ci, V3 d) {
  if (kind == CP_SPHERE) return mkd((double)rec[9], (double)rec[10], (double)rec[11]);
  if (kind == CP_BOX) {
    const M3 R = ldm3(rec);
    const V3 dl = tmulv(R, d);
    const double cx = dl.x >= 0.f ? (double)rec[12] : -(double)rec[12], cy = dl.y >= 0.f ? (double)rec[13] : -(double)rec[13], cz = dl.z >= 0.f ? (double)rec[14] : -(double)rec[14];
    return mkd((double)rec[9] + ((double)R.m[0] * cx + (double)R.m[1] * cy + (double)R.m[2] * cz),
               (double)rec[10] + ((double)R.m[3] * cx + (double)R.m[4] * cy + (double)R.m[5] * cz),
               (double)rec[11] + ((double)R.m[6] * cx + (double)R.m[7] * cy + (double)R.m[8] * cz));
  }
  const M3 R = ldm3(bf);
  const V3 dl = tmulv(R, d);
  const float4* __restrict__ cv = (const float4*)m->hcv;
  const int* __restrict__ co = m->hco + m->hcell_first[ci];
  const int cell = hcell_of(dl);
  const int o0 = co[cell], o1 = co[cell + 1];
  float bd = -1e30f; int bi = 0x7fffffff; float qx = 0.f, qy = 0.f, qz = 0.f;
  for (int k = o0; k < o1; k++) {
    const float4 q = cv[k];
    const float dq = __fmaf_rn(dl.z, q.z, __fmaf_rn(dl.y, q.y, dl.x * q.x));
    const int vi = __float_as_int(q.w);
    if (dq > bd || (dq == bd && vi < bi)) { bd = dq; bi = vi; qx = q.x; qy = q.y; qz = q.z; }
  }
  return mkd((double)bf[9] + ((double)R.m[0] * (double)qx + (double)R.m[1] * (double)qy + (double)R.m[2] * (double)qz),
             (double)bf[10] + ((double)R.m[3] * (double)qx + (double)R.m[4] * (double)qy + (double)R.m[5] * (double)qz),
             (double)bf[11] + ((double)R.m[6] * (double)qx + (double)R.m[7] * (double)qy + (double)R.m[8] * (double)qz));
}

/* one lane's simplex: difference points W, the support points on A, the weights of the closest point; everything in registers (static indices only) */
struct CpSimplex {
  D3 w0, w1, w2, w3, a0, a1, a2, a3;
  double l0, l1, l2;
  int n;
  __device__ __forceinline__ void reduce(D3 p0, D3 p1, D3 p2, D3 q0, D3 q1, D3 q2, int keep, double r0, double r1, double r2) {      /* GjkSimplex::reduce */
    const bool k0 = keep & 1, k1 = keep & 2;
    const double t12 = k1 ? r1 : r2;
    w0 = dsel(k0, p0, dsel(k1, p1, p2)); a0 = dsel(k0, q0, dsel(k1, q1, q2));
    w1 = dsel(k0 && k1, p1, p2); a1 = dsel(k0 && k1, q1, q2);
    w2 = p2; a2 = q2;
    l0 = k0 ? r0 : t12; l1 = (k0 && k1) ? r1 : r2; l2 = r2;
    n = __popc(keep);
  }
  __device__ __forceinline__ D3 mix(D3 p0, D3 p1, D3 p2) const {
    D3 q = dscale(p0, l0);
    if (n > 1) q = dadd(q, dscale(p1, l1));
    if (n > 2) q = dadd(q, dscale(p2, l2));
    return q;
  }
  __device__ __forceinline__ D3 closest() const { return mix(w0, w1, w2); }
  __device__ __forceinline__ D3 on_a() const { return mix(a0, a1, a2); }
  /* closest point of the simplex to the origin; the simplex shrinks to the supporting sub-simplex.  n = 4 afterwards: the origin lies inside the tetrahedron */
  __device__ __forceinline__ void step() {
    if (n == 1) { l0 = 1.0; l1 = 0.0; l2 = 0.0; return; }
    if (n == 2) { const GjkTri r = gjk_seg(w0, w1); reduce(w0, w1, w1, a0, a1, a1, r.keep, r.l0, r.l1, r.l2); return; }
    if (n == 3) { const GjkTri r = gjk_tri(w0, w1, w2); reduce(w0, w1, w2, a0, a1, a2, r.keep, r.l0, r.l1, r.l2); return; }
    double best = 1e30; int bk = 0; double b0 = 0.0, b1 = 0.0, b2 = 0.0;
    D3 pa = w0, pb = w1, pc = w2, qa = a0, qb = a1, qc = a2;
#define CP_FACE(A_, B_, C_, O_, QA_, QB_, QC_) { \
      const D3 nrm = dcross(B_ - A_, C_ - A_); \
      const double so = -ddot(A_, nrm), sd = ddot(O_ - A_, nrm); \
      const bool skip = so * sd > 0.0 || (sd == 0.0 && so == 0.0); \
      const GjkTri r = gjk_tri(A_, B_, C_); \
      const D3 q = mkd(A_.x * r.l0 + B_.x * r.l1 + C_.x * r.l2, A_.y * r.l0 + B_.y * r.l1 + C_.y * r.l2, A_.z * r.l0 + B_.z * r.l1 + C_.z * r.l2); \
      double dd = ddot(q, q); \
      if (skip || !(dd < 1e30)) dd = 1e30; \
      if (dd < best) { best = dd; bk = r.keep; b0 = r.l0; b1 = r.l1; b2 = r.l2; pa = A_; pb = B_; pc = C_; qa = QA_; qb = QB_; qc = QC_; } }
    CP_FACE(w0, w1, w2, w3, a0, a1, a2)
    CP_FACE(w0, w2, w3, w1, a0, a2, a3)
    CP_FACE(w0, w3, w1, w2, a0, a3, a1)
    CP_FACE(w1, w3, w2, w0, a1, a3, a2)
#undef CP_FACE
    if (!(best < 1e30)) return;      /* inside all four faces: n stays 4 */
    reduce(pa, pb, pc, qa, qb, qc, bk, b0, b1, b2);
  }
};

/* one lane per collider of a staged row: the collider's world AABB into ab[6] and, for a hull, its body frame into bf[12] */
__device__ __forceinline__ void cp_stage(const DevModel* __restrict__ m, const float* rec, float* ab, float* bf) {
  const int tw = __float_as_int(rec[18]), ci = __float_as_int(rec[19]) & (RP_MAX_COL - 1);
  float e0, e1, e2;
  if (!(tw & RC_HULL) && (tw & 0xFF) != 0) e0 = e1 = e2 = rec[12];
  else {
    e0 = fabsf(rec[0]) * rec[12] + fabsf(rec[1]) * rec[13] + fabsf(rec[2]) * rec[14];
    e1 = fabsf(rec[3]) * rec[12] + fabsf(rec[4]) * rec[13] + fabsf(rec[5]) * rec[14];
    e2 = fabsf(rec[6]) * rec[12] + fabsf(rec[7]) * rec[13] + fabsf(rec[8]) * rec[14];
  }
  ab[0] = rec[9] - e0; ab[1] = rec[10] - e1; ab[2] = rec[11] - e2; ab[3] = rec[9] + e0; ab[4] = rec[10] + e1; ab[5] = rec[11] + e2;
  if ((tw & RC_HULL) && m->hcell_first[ci] >= 0) {      /* body = record x (collider-to-body)^-1: Rb = R C^T, pb = p - Rb c */
    const float* Cr = m->col_rot[ci]; const float* cp = m->col_pos[ci];
    double Rb[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Rb[3 * i + j] = (double)rec[3 * i] * (double)Cr[3 * j] + (double)rec[3 * i + 1] * (double)Cr[3 * j + 1] + (double)rec[3 * i + 2] * (double)Cr[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 9; i++) bf[i] = (float)Rb[i];
#pragma unroll
    for (int i = 0; i < 3; i++) bf[9 + i] = (float)((double)rec[9 + i] - (Rb[3 * i] * (double)cp[0] + Rb[3 * i + 1] * (double)cp[1] + Rb[3 * i + 2] * (double)cp[2]));
  }
}

/* one pair of a staged row (T: the records, BF: the hulls' body frames, AB: the world AABBs; a != b, both inside the row): status, distance, witnesses, normal */
__device__ __forceinline__ void cp_pair(const DevModel* __restrict__ m, const float* T, const float* BF, const float* AB, int a, int b, float max_distance, int& st,
                                        float& d_out, V3& pa_f, V3& pb_f, V3& n_f) {
  const float* ra = &T[a * RC_STRIDE]; const float* rb = &T[b * RC_STRIDE];
  st = RP_CP_SEPARATED; d_out = 0.f; pa_f = mk3(0, 0, 0); pb_f = mk3(0, 0, 0); n_f = mk3(0, 0, 0);
  bool far = false;
  if (max_distance > 0.f) {      /* the gap of the two world AABBs, a lower bound of the distance */
    const float* A = &AB[6 * a]; const float* B = &AB[6 * b];
    const float gx = fmaxf(fmaxf(A[0] - B[3], B[0] - A[3]), 0.f), gy = fmaxf(fmaxf(A[1] - B[4], B[1] - A[4]), 0.f), gz = fmaxf(fmaxf(A[2] - B[5], B[2] - A[5]), 0.f);
    far = gx * gx + gy * gy + gz * gz > max_distance * max_distance;
  }
  if (far) { st = RP_CP_FAR; d_out = max_distance; }
  else {
    const int twa = __float_as_int(ra[18]), twb = __float_as_int(rb[18]), cia = __float_as_int(ra[19]) & (RP_MAX_COL - 1), cib = __float_as_int(rb[19]) & (RP_MAX_COL - 1);
    const int ka = ((twa & RC_HULL) && m->hcell_first[cia] >= 0) ? CP_HULL : ((twa & RC_HULL) || (twa & 0xFF) == 0 ? CP_BOX : CP_SPHERE);
    const int kb = ((twb & RC_HULL) && m->hcell_first[cib] >= 0) ? CP_HULL : ((twb & RC_HULL) || (twb & 0xFF) == 0 ? CP_BOX : CP_SPHERE);
    const float* bfa = &BF[12 * a]; const float* bfb = &BF[12 * b];
    const double rad_a = ka == CP_SPHERE ? (double)ra[12] : 0.0, rad_b = kb == CP_SPHERE ? (double)rb[12] : 0.0;
    CpSimplex S;
    V3 d0 = ld3(ra + 9) - ld3(rb + 9);
    if (d0.x == 0.f && d0.y == 0.f && d0.z == 0.f) d0 = mk3(1.f, 0.f, 0.f);
    S.a0 = cp_support(m, ka, ra, bfa, cia, -d0);
    S.w0 = S.a0 - cp_support(m, kb, rb, bfb, cib, d0);
    S.w1 = S.w2 = S.w3 = S.w0; S.a1 = S.a2 = S.a3 = S.a0;
    S.n = 1; S.l0 = 1.0; S.l1 = 0.0; S.l2 = 0.0;
    D3 v = S.w0; double dd = ddot(v, v);
    bool overlap = dd < GJK_ZERO, done = false;
#pragma unroll 1
    for (int it = 0; it < RP_CP_ITERS && !overlap; it++) {
      const V3 vf = mk3((float)v.x, (float)v.y, (float)v.z);
      const D3 sa = cp_support(m, ka, ra, bfa, cia, -vf);
      const D3 w = sa - cp_support(m, kb, rb, bfb, cib, vf);
      const double vv = ddot(v, v), vw = ddot(v, w);
      bool dup = false;
      { D3 dw = S.w0 - w; dup |= ddot(dw, dw) < GJK_DUP;
        dw = S.w1 - w; dup |= S.n > 1 && ddot(dw, dw) < GJK_DUP;
        dw = S.w2 - w; dup |= S.n > 2 && ddot(dw, dw) < GJK_DUP; }
      if (dup || vv - vw <= GJK_REL * vv) { done = true; break; }
      if (S.n == 1) { S.w1 = w; S.a1 = sa; } else if (S.n == 2) { S.w2 = w; S.a2 = sa; } else { S.w3 = w; S.a3 = sa; }
      S.n++;
      S.step();
      if (S.n == 4) { overlap = true; break; }
      v = S.closest();
      const double nd = ddot(v, v);
      if (nd < GJK_ZERO) { overlap = true; break; }
      if (nd >= dd * GJK_STALL) { dd = nd; done = true; break; }
      dd = nd;
    }
    D3 xa, xb, nn = mkd(0, 0, 0);
    if (S.n == 4) {      /* the origin inside the tetrahedron: its barycentric coordinates give the common point */
      const D3 e1 = S.w1 - S.w0, e2 = S.w2 - S.w0, e3 = S.w3 - S.w0, o = mkd(-S.w0.x, -S.w0.y, -S.w0.z);
      const double vol = ddot(e1, dcross(e2, e3));
      double m1 = ddot(o, dcross(e2, e3)), m2 = ddot(e1, dcross(o, e3)), m3 = ddot(e1, dcross(e2, o));
      const double iv = vol != 0.0 ? 1.0 / vol : 0.0;
      m1 = fmin(fmax(m1 * iv, 0.0), 1.0); m2 = fmin(fmax(m2 * iv, 0.0), 1.0); m3 = fmin(fmax(m3 * iv, 0.0), 1.0);
      double m0 = fmax(1.0 - m1 - m2 - m3, 0.0);
      if (vol == 0.0) { m0 = m1 = m2 = m3 = 0.25; }
      const double sc = 1.0 / (m0 + m1 + m2 + m3);
      xa = dscale(dadd(dadd(dscale(S.a0, m0), dscale(S.a1, m1)), dadd(dscale(S.a2, m2), dscale(S.a3, m3))), sc);
      xb = xa;
    } else {
      xa = S.on_a();
      xb = overlap ? xa : xa - v;
    }
    const double dc = overlap ? 0.0 : sqrt(ddot(v, v));
    const double dsep = dc - rad_a - rad_b;
    if (overlap || !(dsep > 0.0)) {      /* the cores overlap, or the spheres' radii cover the cores' gap: a point within rad_a of A's core and rad_b of B's */
      st = RP_CP_OVERLAP;
      if (!overlap && dc > 0.0 && rad_a + rad_b > 0.0) { const double t = rad_a / (rad_a + rad_b); xa = mkd(xa.x - v.x * t, xa.y - v.y * t, xa.z - v.z * t); }
      xb = xa;
      d_out = 0.f;
    } else {
      const double inv = 1.0 / dc;
      nn = dscale(v, inv);
      xa = xa - dscale(nn, rad_a);
      xb = dadd(xb, dscale(nn, rad_b));
      d_out = (float)dsep;
      if (!done) st |= RP_CP_CAPPED;
    }
    pa_f = mk3((float)xa.x, (float)xa.y, (float)xa.z); pb_f = mk3((float)xb.x, (float)xb.y, (float)xb.z); n_f = mk3((float)nn.x, (float)nn.y, (float)nn.z);
  }
}

/* Row `slot` of the launch = row row_index[slot] (null: base + slot) of the caller's buffer, whose records k_collider_poses_rows left in slot `slot` of tab / cnt; a row
 * outside [0, n_rows) has no records (the pose kernel left before it wrote): every pair of it is RP_CP_SKIPPED.  pairs [K][3]: collider a, collider b, group.  The outputs
 * (each may be null) start at the launch's first row: dist / status [num][K], pa / pb / nrm [num][K][3], gmin / gpair [num][G].  A SKIPPED pair writes its status alone.
 * Dynamic LDS: G * 64 floats and G * 64 ints - every lane's running minimum per group, joined per group at the end (the smallest distance, the lowest pair index
 * among equals: the result of a scan in pair order). */
__global__ void __launch_bounds__(64) k_closest_points(const DevModel* __restrict__ m, const float* __restrict__ tab, const int* __restrict__ cnt, int num,
                                                       const int* __restrict__ row_index, int base, int n_rows, const int* __restrict__ pairs, int K, int G,
                                                       float max_distance, float* __restrict__ dist, float* __restrict__ pa_out, float* __restrict__ pb_out,
                                                       float* __restrict__ nrm_out, int* __restrict__ status, float* __restrict__ gmin, int* __restrict__ gpair) {
  __shared__ float T[RP_MAX_COL * RC_STRIDE];
  __shared__ float BF[RP_MAX_COL * 12];
  __shared__ float AB[RP_MAX_COL * 6];
  extern __shared__ float GL[];
  const int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= num) return;
  const int row = row_index ? row_index[slot] : base + slot;
  const bool has_row = row >= 0 && row < n_rows;                     /* block-uniform */
  const bool groups = G > 0 && (gmin || gpair);
  float* gl_min = GL; int* gl_idx = (int*)(GL + 64 * G);
  if (groups)
    for (int g = 0; g < G; g++) { gl_min[64 * g + lane] = __int_as_float(0x7f800000); gl_idx[64 * g + lane] = -1; }
  int n = 0;
  if (has_row) {
    n = min(min(cnt[slot], m->n_col), RP_MAX_COL);
    for (int i = lane; i < n * RC_STRIDE; i += 64) T[i] = tab[(size_t)slot * RC_MAX * RC_STRIDE + i];
  }
  __syncthreads();
  if (lane < n) {
    cp_stage(m, &T[lane * RC_STRIDE], &AB[6 * lane], &BF[12 * lane]);
  }
  __syncthreads();
  for (int k = lane; k < K; k += 64) {
    const size_t r = (size_t)slot * K + k;
    const int a = pairs[3 * k], b = pairs[3 * k + 1], g = pairs[3 * k + 2];
    if (!has_row || a < 0 || a >= n || b < 0 || b >= n || a == b) { if (status) status[r] = RP_CP_SKIPPED; continue; }
    int st; float d_out; V3 pa_f, pb_f, n_f;
    cp_pair(m, T, BF, AB, a, b, max_distance, st, d_out, pa_f, pb_f, n_f);
    if (dist) dist[r] = d_out;
    if (pa_out) st3(pa_out + 3 * r, pa_f);
    if (pb_out) st3(pb_out + 3 * r, pb_f);
    if (nrm_out) st3(nrm_out + 3 * r, n_f);
    if (status) status[r] = st;
    if (groups && g >= 0 && g < G && d_out < gl_min[64 * g + lane]) { gl_min[64 * g + lane] = d_out; gl_idx[64 * g + lane] = k; }      /* (a lane's pairs rise: its first strict minimum is its lowest index) */
  }
  if (!groups) return;
  __syncthreads();
  if (lane < G) {
    float best = __int_as_float(0x7f800000); int bi = -1;
    for (int j = 0; j < 64; j++) {
      const int c = (j + lane) & 63;      /* (rotated: the lanes read different banks) */
      const float v = gl_min[64 * lane + c]; const int i = gl_idx[64 * lane + c];
      if (i >= 0 && (bi < 0 || v < best || (v == best && i < bi))) { best = v; bi = i; }
    }
    if (gmin) gmin[(size_t)slot * G + lane] = best;
    if (gpair) gpair[(size_t)slot * G + lane] = bi;
  }
}
