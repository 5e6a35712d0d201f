// k_pgo.hip -- pose-graph optimisation (include/pose_graph.h): batched Levenberg-Marquardt over
// relative-pose edges, the damped normal equations solved by a scalar Cholesky inside the row
// envelope.
//
// k_pg_solve: one 256-thread workgroup per graph, a grid-stride loop over the graphs, a scratch slab
// per workgroup (so scratch scales with the grid) beside one linearisation per stored edge, kept by
// the global edge index (640 B an edge).  No communication between workgroups, every loop is
// bounded by an argument, no float atomics (and no integer ones either).  Per graph:
//   prologue   copy the state through; check the offsets and every edge; a thread per node walks the
//              graph's edges in order: its degree, then (after a scan) its incidence list in
//              ascending edge index; the free nodes numbered by a workgroup scan; first[] by a
//              thread per free node, the envelope offsets by a scan; per block column the block rows
//              below the diagonal that reach it (count, scan, fill, ascending).
//   linearise  a thread per edge: e, the 6 x 12 Jacobian and the IRLS weight to the slab, the cost by
//              the contract's fixed tree.  Only at the start and after an accepted step.
//   per solve, a barrier between the phases:
//     (a) an owner per entry of every block inside the envelope adds its node's edges in incidence
//         order (the diagonal block: all of them; an off-diagonal block: those of the pair), damps
//         the diagonal; an owner per entry of b.
//     (b) right-looking Cholesky, a block column (six scalar columns) at a time.  The rows below
//         the diagonal block that reach it are the block rows of its column list (staged in LDS).
//         Phase 1: every thread factors the 6 x 6 diagonal block for itself in registers (thread 0
//         stores it and finishes the six y); a thread per row below carries its six entries through
//         the six columns.  Phase 2: a thread per pair of those rows subtracts its six terms
//         L[r][j] L[c][j] in turn from H[r][c], a thread per row its six L[r][j] y[j] from b[r].
//         Every entry so receives its terms in ascending k, as the left-looking formula of the
//         contract does; the right-hand side rides along.
//     (c) back substitution, block column by block column downwards: a thread per entry below the
//         diagonal block multiplies L[k][i] x[k], thread 0 subtracts the products in ascending k and
//         divides (the products are rounded on their own, so this is the serial sum's bits).
//     (d) candidate poses (rounded once to fp32) into the slab, the candidate's cost.
//     (e) thread 0 decides and broadcasts through LDS; an accepted candidate is copied to the output.
// The loss, the cost tree, the pose retraction and the decision are mv_lm.hpp's, shared with
// k_ba_solve and k_pnp_solve; the prologue's scans are tr_scan.hpp's, a barrier after each.
// All arithmetic is float64 in the order of tests/pgo_reference.py (-ffp-contract=off).
// The factor lives in the slab (env_cap x 36 doubles) and every block column goes through it: one
// read and one write of the slab per phase.  LDS holds b / y / x and the back substitution's
// products (2 x 6 x nodes doubles; a column that more than nodes / 6 block rows reach puts its
// products in the slab instead) and the bookkeeping that finds the rows: first / envoff / colptr of
// the graph and the current block column's list, 5 x nodes ints.  29.1 KiB at 257 nodes, 58 KiB at
// the limit of 512, plus 2 KiB for the cost tree and 1 KiB for the scans.  A graph per wave with
// several graphs per workgroup was not taken: a block column's pair updates are what there is to
// spread (21 per block row pair), and at 257 nodes a graph's LDS alone is a wave's fair share.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "mv_internal.hpp"
#include "mv_lm.hpp"
#include "mv_quat.hpp"
#include "pose_graph.h"
#include "tr_scan.hpp"

namespace {

using mv::dmax;
using mv::qmul;

constexpr int NT = 256;

// The edge arrays are indexed by the global edge: the graphs that solve own disjoint edge ranges (an
// edge's node ids are valid for one graph only, and a graph with an invalid edge never writes).
// Every other array: one per kind for the whole grid; workgroup g uses slice g of each.
struct PgScratch {
    double *A;     // [ecap][72]         Jacobian of every edge, row-major 6 x 12
    double *ev;    // [ecap][6]          error
    double *wt;    // [ecap]             IRLS weight
    int *inc;      // [2 ecap]           incidence lists, a graph's at twice its first edge
    double *env;   // [grid][envc][36]   H, then L: the blocks inside the envelope, row by row
    double *Ld;    // [grid][N][36]      the factored diagonal blocks
    double *prod;  // [grid][N][36]      back substitution's products where LDS is too small for them
    float *cP;     // [grid][N][7]       candidate poses
    int *nodeoff;  // [grid][N + 1]      a node's part of the graph's incidence lists
    int *fidx;     // [grid][N]          free number or -1
    int *fnode;    // [grid][N]          node of a free number
    int *first;    // [grid][N]
    int *envoff;   // [grid][N + 1]      first block of a block row
    int *colptr;   // [grid][N + 1]      block rows below the diagonal that reach a block column
    int *colrow;   // [grid][envc]
};

PgScratch pg_scratch_layout(mv::Carve &c, size_t grid, size_t ecap, size_t envc, size_t N) {
    PgScratch m;
    m.A = c.take<double>(ecap * 72);
    m.ev = c.take<double>(ecap * 6);
    m.wt = c.take<double>(ecap);
    m.inc = c.take<int>(ecap * 2);
    m.env = c.take<double>(grid * envc * 36);
    m.Ld = c.take<double>(grid * N * 36);
    m.prod = c.take<double>(grid * N * 36);
    m.cP = c.take<float>(grid * N * 7);
    m.nodeoff = c.take<int>(grid * (N + 1));
    m.fidx = c.take<int>(grid * N);
    m.fnode = c.take<int>(grid * N);
    m.first = c.take<int>(grid * N);
    m.envoff = c.take<int>(grid * (N + 1));
    m.colptr = c.take<int>(grid * (N + 1));
    m.colrow = c.take<int>(grid * envc);
    return m;
}

// x, y: columns of a row-major 6 x 12 Jacobian (stride 12), or y = the error (stride 1)
__device__ __forceinline__ double dot6(const double *x, const double *y, int ystride) {
    return ((((x[0] * y[0] + x[12] * y[ystride]) + x[24] * y[2 * ystride]) + x[36] * y[3 * ystride]) +
            x[48] * y[4 * ystride]) +
           x[60] * y[5 * ystride];
}

// One edge at the fp32 poses pi, pj: e [6], and with A != nullptr the Jacobian [6][12].
__device__ void edge_residual(const float *pi, const float *pj, int kind, const float *z, const float *w, double *e,
                              double *A) {
    const double qi[4] = {pi[0], pi[1], pi[2], pi[3]}, ti[3] = {pi[4], pi[5], pi[6]};
    const double qj[4] = {pj[0], pj[1], pj[2], pj[3]}, tj[3] = {pj[4], pj[5], pj[6]};
    const double qz[4] = {z[0], z[1], z[2], z[3]}, tz[3] = {z[4], z[5], z[6]};
    const double wr = w[0], wt = w[1];
    const double ci[4] = {qi[0], -qi[1], -qi[2], -qi[3]}, cz[4] = {qz[0], -qz[1], -qz[2], -qz[3]};
    double qp[4], R[9], qe[4];
    qmul(qj, ci, qp);
    mv::quat_rot(qp, R);
    const double tp[3] = {tj[0] - ((R[0] * ti[0] + R[1] * ti[1]) + R[2] * ti[2]),
                          tj[1] - ((R[3] * ti[0] + R[4] * ti[1]) + R[5] * ti[2]),
                          tj[2] - ((R[6] * ti[0] + R[7] * ti[1]) + R[8] * ti[2])};
    qmul(cz, qp, qe);
    const double sg = qe[0] < 0.0 ? -1.0 : 1.0;
    const double rr[3] = {(2.0 * sg) * qe[1], (2.0 * sg) * qe[2], (2.0 * sg) * qe[3]};
    double P[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double rt[3];
    if (kind == MV_PG_EDGE_SE3) {
        rt[0] = tp[0] - tz[0], rt[1] = tp[1] - tz[1], rt[2] = tp[2] - tz[2];
    } else {
        const double n2 = (tp[0] * tp[0] + tp[1] * tp[1]) + tp[2] * tp[2];
        if (n2 > 0.0) {
            const double nn = sqrt(n2);
            const double u[3] = {tp[0] / nn, tp[1] / nn, tp[2] / nn};
            rt[0] = u[0] - tz[0], rt[1] = u[1] - tz[1], rt[2] = u[2] - tz[2];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) P[a][b] = (P[a][b] - u[a] * u[b]) / nn;
        } else {
            rt[0] = rt[1] = rt[2] = 0.0;
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) P[a][b] = 0.0;
        }
    }
    const double sr = sqrt(wr), st = sqrt(wt);
    e[0] = sr * rr[0], e[1] = sr * rr[1], e[2] = sr * rr[2];
    e[3] = st * rt[0], e[4] = st * rt[1], e[5] = st * rt[2];
    if (!A) return;
    const double qw = qe[0], v0 = qe[1], v1 = qe[2], v2 = qe[3];
    const double K[3][3] = {{qw, -v2, v1}, {v2, qw, -v0}, {-v1, v0, qw}};
    const double X[3][3] = {{0.0, -tp[2], tp[1]}, {tp[2], 0.0, -tp[0]}, {-tp[1], tp[0], 0.0}};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            A[12 * r + c] = -(sr * (sg * K[r][c]));
            A[12 * r + 3 + c] = 0.0;
            A[12 * r + 6 + c] = sr * (sg * ((K[r][0] * R[3 * c] + K[r][1] * R[3 * c + 1]) + K[r][2] * R[3 * c + 2]));
            A[12 * r + 9 + c] = 0.0;
            A[12 * (3 + r) + c] = 0.0;
            A[12 * (3 + r) + 3 + c] = -(st * ((P[r][0] * R[c] + P[r][1] * R[3 + c]) + P[r][2] * R[6 + c]));
            A[12 * (3 + r) + 6 + c] = -(st * ((P[r][0] * X[0][c] + P[r][1] * X[1][c]) + P[r][2] * X[2][c]));
            A[12 * (3 + r) + 9 + c] = st * P[r][c];
        }
}

// the graph's view of one workgroup
struct Gr {
    int base, e0, E;  // first global node id, first edge, edges
    const int *ei, *ej, *kind;
    const float *z, *w;
    double *A, *ev, *wt;
};

// Linearise the graph's edges at poses [N][7] -- jac: A, e and the weight to the slab -- and return
// the cost in *out (LDS) by the fixed tree.  Ends with a barrier.
__device__ void linearize(const Gr &G, const float *poses, bool jac, double huber, double *s_part, double *out) {
    const int tid = threadIdx.x;
    double part = 0.0;
    for (int k = tid; k < G.E; k += NT) {
        const size_t g = (size_t)G.e0 + k;
        const int i = G.ei[g] - G.base, j = G.ej[g] - G.base;  // validated in the prologue
        double e[6];
        edge_residual(poses + 7l * i, poses + 7l * j, G.kind[g], G.z + 7 * g, G.w + 2 * g, e,
                      jac ? G.A + 72 * (size_t)k : nullptr);
        const double s = ((((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]) + e[4] * e[4]) + e[5] * e[5];
        double rho, wt;
        mv::huber_loss(s, huber, rho, wt);
        part = part + rho;
        if (jac) {
#pragma unroll
            for (int c = 0; c < 6; c++) G.ev[6 * (size_t)k + c] = e[c];
            G.wt[k] = wt;
        }
    }
    mv::tree_sum_256(part, s_part, out);
}

__global__ __launch_bounds__(NT) void k_pg_solve(mv_pg_params P, int batch, int N, int num_edges, int env_cap,
                                                 const float *pin, const int *__restrict__ offs,
                                                 const int *__restrict__ ei, const int *__restrict__ ej,
                                                 const int *__restrict__ ekind, const float *__restrict__ ez,
                                                 const float *__restrict__ ew, const int *__restrict__ fixed,
                                                 float *pout, double *__restrict__ cost0, double *__restrict__ cost1,
                                                 int *__restrict__ iters, int *__restrict__ status, PgScratch scr,
                                                 int envc) {
    // s_col [6 N] (back substitution's products), b / y / x [6 N]; then ints: first [N], envoff [N + 1],
    // colptr [N + 1], and of the current block column's list: block row [N], and where that row's
    // blocks would start in the slab if the row began at block column 0 [N]
    extern __shared__ double s_dyn[];
    __shared__ double s_part[NT];
    __shared__ int s_scan[NT];
    __shared__ int s_e0, s_e1, s_fail, s_iters;
    __shared__ mv::LmState s_lm;
    __shared__ double s_cand;
    const int tid = threadIdx.x;
    const size_t wg = blockIdx.x;
    double *const env = scr.env + wg * (size_t)envc * 36;
    double *const Ldg = scr.Ld + wg * (size_t)N * 36;
    double *const prodg = scr.prod + wg * (size_t)N * 36;
    float *const cP = scr.cP + wg * (size_t)N * 7;
    int *const nodeoff = scr.nodeoff + wg * (size_t)(N + 1);
    int *const fidx = scr.fidx + wg * (size_t)N;
    int *const fnode = scr.fnode + wg * (size_t)N;
    int *const first = scr.first + wg * (size_t)N;
    int *const envoff = scr.envoff + wg * (size_t)(N + 1);
    int *const colptr = scr.colptr + wg * (size_t)(N + 1);
    int *const colrow = scr.colrow + wg * (size_t)envc;
    double *const s_col = s_dyn, *const xs = s_dyn + 6 * N;
    int *const s_first = reinterpret_cast<int *>(s_dyn + 12 * N), *const s_envoff = s_first + N;
    int *const s_colptr = s_envoff + N + 1, *const s_kb = s_colptr + N + 1, *const s_rb = s_kb + N;
    // row p of the staged list: six rows per entry
    auto row_of = [&](int p, int &kb, int &a, int &rb) {
        const int q = p / 6;
        kb = s_kb[q], a = p - 6 * q, rb = s_rb[q];
    };
    // the list of block column cb into LDS; the caller puts a barrier before and after
    auto stage_list = [&](int cb) {
        const int c0 = s_colptr[cb], cnt = s_colptr[cb + 1] - c0;
        for (int q = tid; q < cnt; q += NT) {
            const int kb = colrow[c0 + q];
            s_kb[q] = kb;
            s_rb[q] = (s_envoff[kb] - s_first[kb]) * 36;
        }
    };

    for (int s = blockIdx.x; s < batch; s += gridDim.x) {
        __syncthreads();  // the previous graph's shared state is done with
        if (tid == 0) {
            s_e0 = offs[s], s_e1 = offs[s + 1];
            mv::lm_reset(s_lm, P.lambda_init);
            s_fail = 0, s_iters = 0;
        }
        const float *Pi = pin + (size_t)s * N * 7;
        float *Po = pout + (size_t)s * N * 7;
        for (int i = tid; i < N * 7; i += NT) Po[i] = Pi[i];
        __syncthreads();

        int st = MV_OK;
        const int e0 = s_e0, e1 = s_e1, base = s * N;
        if (e0 < 0 || e1 < e0)
            st = MV_ERR_INVALID_ARG;
        else if (e1 > num_edges)
            st = MV_ERR_CAPACITY;
        const int E = st == MV_OK ? e1 - e0 : 0;  // e0 + E <= num_edges <= ecap
        double *const Af = scr.A + (size_t)(E ? e0 : 0) * 72, *const evf = scr.ev + (size_t)(E ? e0 : 0) * 6;
        double *const wf = scr.wt + (E ? e0 : 0);
        int *const inc = scr.inc + 2 * (size_t)(E ? e0 : 0);
        int bad = 0;
        for (int k = tid; k < E; k += NT) {
            const size_t g = (size_t)e0 + k;
            const long i = (long)ei[g] - base, j = (long)ej[g] - base;
            const int kd = ekind[g];
            const float w0 = ew[2 * g], w1 = ew[2 * g + 1];
            if (i < 0 || i >= N || j < 0 || j >= N || i == j || (kd != MV_PG_EDGE_SE3 && kd != MV_PG_EDGE_DIRECTION) ||
                !(w0 >= 0.0f) || !(w1 >= 0.0f) || !isfinite(w0) || !isfinite(w1))
                bad = 1;
        }
        if (__syncthreads_or(bad)) st = MV_ERR_INVALID_ARG;

        int nfree = 0, envtot = 0;
        if (st == MV_OK && E > 0) {  // uniform over the workgroup
            // degrees, then the incidence lists in ascending edge index: a thread per node
            for (int n = tid; n < N; n += NT) {
                int cnt = 0;
                for (int k = 0; k < E; k++) cnt += (ei[e0 + k] - base == n) | (ej[e0 + k] - base == n);
                nodeoff[n] = cnt;
            }
            if (tid == 0) nodeoff[N] = 0;
            __syncthreads();
            tr::scan_exclusive_256(N + 1, nodeoff, s_scan);
            __syncthreads();
            for (int n = tid; n < N; n += NT) {
                int p = nodeoff[n];
                for (int k = 0; k < E; k++)
                    if (ei[e0 + k] - base == n || ej[e0 + k] - base == n) inc[p++] = k;
                const int held = (fixed ? fixed[(size_t)base + n] != 0 : n == 0) || nodeoff[n + 1] == nodeoff[n];
                colptr[n] = !held;  // kept beside the scan of the same flags
                fidx[n] = !held;
            }
            __syncthreads();
            nfree = tr::scan_exclusive_256(N, fidx, s_scan);
            __syncthreads();
            for (int n = tid; n < N; n += NT) {
                if (colptr[n])
                    fnode[fidx[n]] = n;
                else
                    fidx[n] = -1;
            }
            __syncthreads();
            if (nfree == 0) st = MV_ERR_DEGENERATE;
        }
        if (st == MV_OK && E > 0) {
            for (int k = tid; k < nfree; k += NT) {
                const int nd = fnode[k];
                int lo = k;
                for (int p = nodeoff[nd]; p < nodeoff[nd + 1]; p++) {
                    const int e = inc[p], gi = ei[e0 + e] - base, gj = ej[e0 + e] - base;
                    const int o = fidx[gi == nd ? gj : gi];
                    if (o >= 0 && o < lo) lo = o;
                }
                first[k] = lo;
                envoff[k] = k - lo + 1;
            }
            if (tid == 0) envoff[nfree] = 0;
            __syncthreads();
            envtot = tr::scan_exclusive_256(nfree + 1, envoff, s_scan);
            __syncthreads();
            if (envtot > env_cap) st = MV_ERR_CAPACITY;  // envtot <= N (N + 1) / 2 <= envc otherwise
        }
        if (st != MV_OK || E == 0) {  // uniform
            if (tid == 0) {
                status[s] = st;
                iters[s] = 0;
                cost0[s] = 0.0;
                cost1[s] = 0.0;
            }
            continue;
        }
        // per block column, the block rows below the diagonal that reach it, ascending
        for (int cb = tid; cb < nfree; cb += NT) {
            int cnt = 0;
            for (int kb = cb + 1; kb < nfree; kb++) cnt += first[kb] <= cb;
            colptr[cb] = cnt;
        }
        if (tid == 0) colptr[nfree] = 0;
        __syncthreads();
        tr::scan_exclusive_256(nfree + 1, colptr, s_scan);  // total = envtot - nfree
        __syncthreads();
        for (int cb = tid; cb < nfree; cb += NT) {
            int p = colptr[cb];
            for (int kb = cb + 1; kb < nfree; kb++)
                if (first[kb] <= cb) colrow[p++] = kb;
        }
        __syncthreads();
        for (int k = tid; k <= nfree; k += NT) {
            if (k < nfree) s_first[k] = first[k];
            s_envoff[k] = envoff[k], s_colptr[k] = colptr[k];
        }
        __syncthreads();

        const int n = 6 * nfree;
        Gr G{base, e0, E, ei, ej, ekind, ez, ew, Af, evf, wf};
        linearize(G, Po, true, P.huber, s_part, &s_lm.cost);
        const double c_init = s_lm.cost;

        for (int it = 0; it < P.max_iters; it++) {
            if (s_lm.stop) break;  // uniform: written before the last barrier
            if (s_lm.relin) linearize(G, Po, true, P.huber, s_part, &s_lm.cost);
            const double lam = s_lm.lambda, floor_ = P.diag_floor;

            // (a) H inside the envelope and b
            for (int t = tid; t < envtot * 36; t += NT) {
                const int blk = t / 36, q = t - blk * 36, a = q / 6, bb = q - a * 6;
                int lo = 0, hi = nfree - 1;  // the block row that holds blk: envoff[k] <= blk < envoff[k + 1]
                for (int step = 0; step < 10 && lo < hi; step++) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_envoff[mid] <= blk)
                        lo = mid;
                    else
                        hi = mid - 1;
                }
                const int k = lo, c = s_first[k] + (blk - s_envoff[k]);
                if (c == k && bb > a) continue;  // the upper triangle is never read
                const int nd = fnode[k], nc = fnode[c];
                double acc = 0.0;
                for (int p = nodeoff[nd]; p < nodeoff[nd + 1]; p++) {
                    const int e = inc[p], gi = ei[e0 + e] - base, gj = ej[e0 + e] - base;
                    const double *Ae = Af + 72 * (size_t)e + (gi == nd ? 0 : 6);
                    if (c == k)
                        acc = acc + wf[e] * dot6(Ae + a, Ae + bb, 12);
                    else if (gi == nc || gj == nc)
                        acc = acc + wf[e] * dot6(Ae + a, Af + 72 * (size_t)e + (gi == nc ? 0 : 6) + bb, 12);
                }
                if (c == k && a == bb) acc = acc + lam * dmax(acc, floor_);
                env[(size_t)t] = acc;
            }
            for (int t = tid; t < n; t += NT) {
                const int k = t / 6, a = t - k * 6, nd = fnode[k];
                double acc = 0.0;
                for (int p = nodeoff[nd]; p < nodeoff[nd + 1]; p++) {
                    const int e = inc[p], gi = ei[e0 + e] - base;
                    acc = acc - wf[e] * dot6(Af + 72 * (size_t)e + (gi == nd ? 0 : 6) + a, evf + 6 * (size_t)e, 1);
                }
                xs[t] = acc;
            }
            // (b) right-looking Cholesky, a block column (six scalar columns) at a time; b rides along
            // and leaves as y
            for (int cb = 0; cb < nfree; cb++) {
                __syncthreads();
                stage_list(cb);
                __syncthreads();
                const int j0 = 6 * cb, m = 6 * (s_colptr[cb + 1] - s_colptr[cb]);
                const int own = (s_envoff[cb] - s_first[cb] + cb) * 36;  // the diagonal block
                // the diagonal block, by every thread for itself: column by column, as the scalar
                // right-looking sweep orders it
                double D[6][6];
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = 0; b <= a; b++) D[a][b] = env[own + a * 6 + b];
                bool bad = false;
#pragma unroll
                for (int jj = 0; jj < 6; jj++) {
                    const double d = D[jj][jj];
                    if (!(d > 0.0) || !isfinite(d)) bad = true;
                    const double dd = sqrt(d);
                    D[jj][jj] = dd;
#pragma unroll
                    for (int a = jj + 1; a < 6; a++) D[a][jj] = D[a][jj] / dd;
#pragma unroll
                    for (int a = jj + 1; a < 6; a++)
#pragma unroll
                        for (int b = jj + 1; b <= a; b++) D[a][b] = D[a][b] - D[a][jj] * D[b][jj];
                }
                if (tid == 0) {
                    if (bad) s_fail = 1;
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int b = 0; b <= a; b++) Ldg[36 * cb + a * 6 + b] = D[a][b];
#pragma unroll
                    for (int jj = 0; jj < 6; jj++) {
                        const double y = xs[j0 + jj] / D[jj][jj];
                        xs[j0 + jj] = y;
#pragma unroll
                        for (int a = jj + 1; a < 6; a++) xs[j0 + a] = xs[j0 + a] - D[a][jj] * y;
                    }
                }
                // phase 1: a thread per row below: its six entries of the block column
                for (int p = tid; p < m; p += NT) {
                    int kb, a, rb;
                    row_of(p, kb, a, rb);
                    double *h = env + rb + cb * 36 + a * 6;
                    double l[6];
#pragma unroll
                    for (int jj = 0; jj < 6; jj++) l[jj] = h[jj];
#pragma unroll
                    for (int jj = 0; jj < 6; jj++) {
                        l[jj] = l[jj] / D[jj][jj];
#pragma unroll
                        for (int c = jj + 1; c < 6; c++) l[c] = l[c] - l[jj] * D[c][jj];
                    }
#pragma unroll
                    for (int jj = 0; jj < 6; jj++) h[jj] = l[jj];
                }
                __syncthreads();
                // phase 2: every row's right-hand side and every pair of rows, the six terms in turn
                for (int p = tid; p < m; p += NT) {
                    int kb, a, rb;
                    row_of(p, kb, a, rb);
                    const double *l = env + rb + cb * 36 + a * 6;
                    double v = xs[6 * kb + a];
#pragma unroll
                    for (int jj = 0; jj < 6; jj++) v = v - l[jj] * xs[j0 + jj];
                    xs[6 * kb + a] = v;
                }
                for (int t = tid; t < m * (m + 1) / 2; t += NT) {
                    int pr = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);  // pr (pr + 1) / 2 <= t
                    if ((pr + 1) * (pr + 2) / 2 <= t) pr++;
                    if (pr * (pr + 1) / 2 > t) pr--;
                    const int pc = t - pr * (pr + 1) / 2;  // pc <= pr: row pr, column = row pc
                    int kb, a, rb, kc, b, rc;
                    row_of(pr, kb, a, rb);
                    row_of(pc, kc, b, rc);
                    const double *lr = env + rb + cb * 36 + a * 6, *lc = env + rc + cb * 36 + b * 6;
                    double *h = env + rb + kc * 36 + a * 6 + b;
                    double v = *h;
#pragma unroll
                    for (int jj = 0; jj < 6; jj++) v = v - lr[jj] * lc[jj];
                    *h = v;
                }
            }
            // (c) back substitution, a block column at a time downwards: the products in parallel,
            // their subtraction in ascending k by thread 0
            for (int cb = nfree - 1; cb >= 0; cb--) {
                __syncthreads();
                stage_list(cb);
                __syncthreads();
                const int j0 = 6 * cb, m = 6 * (s_colptr[cb + 1] - s_colptr[cb]);
                double *const pr = m <= N ? s_col : prodg;  // [m][6]
                for (int t = tid; t < 6 * m; t += NT) {
                    const int p = t / 6, jj = t - 6 * p;
                    int kb, a, rb;
                    row_of(p, kb, a, rb);
                    pr[t] = env[rb + cb * 36 + a * 6 + jj] * xs[6 * kb + a];
                }
                __syncthreads();
                if (tid == 0) {
                    const double *D = Ldg + 36 * cb;
                    for (int jj = 5; jj >= 0; jj--) {
                        double acc = xs[j0 + jj];
                        for (int a = jj + 1; a < 6; a++) acc = acc - D[a * 6 + jj] * xs[j0 + a];
                        for (int p = 0; p < m; p++) acc = acc - pr[6 * p + jj];
                        xs[j0 + jj] = acc / D[jj * 6 + jj];
                    }
                }
            }
            __syncthreads();
            // (d) the candidate state
            for (int f = tid; f < N; f += NT) {
                const int fi = fidx[f];
                if (fi < 0) {
                    for (int c = 0; c < 7; c++) cP[7 * f + c] = Po[7 * f + c];
                    continue;
                }
                mv::retract_pose(xs + 6 * fi, Po + 7 * f, cP + 7 * f);
            }
            __syncthreads();
            linearize(G, cP, false, P.huber, s_part, &s_cand);
            // (e) the decision
            if (tid == 0) {
                s_iters = s_iters + 1;
                mv::lm_decide(P, s_lm, s_fail != 0, s_cand);
                s_fail = 0;
            }
            __syncthreads();
            if (s_lm.acc)
                for (int i = tid; i < N * 7; i += NT) Po[i] = cP[i];
            __syncthreads();
        }
        if (tid == 0) {
            status[s] = MV_OK;
            iters[s] = s_iters;
            cost0[s] = c_init;
            cost1[s] = s_lm.cost;
        }
    }
}

// poses_to_q7's arithmetic (mvtrack.py) in float64, a thread per transform
__global__ void k_pg_edges_from_transforms(int E, const float *__restrict__ T, float *__restrict__ z) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= E) return;
    double R[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = T[12l * k + 4 * r + c];
        t[r] = T[12l * k + 4 * r + 3];
    }
    double q[4];
    mv::rot_to_quat(R, q);
    for (int i = 0; i < 4; i++) z[7l * k + i] = (float)q[i];
    for (int i = 0; i < 3; i++) z[7l * k + 4 + i] = (float)t[i];
}

}  // namespace

extern "C" void mv_pg_params_default(mv_pg_params *p) {
    if (!p) return;
    mv::lm_params_default(p);
    p->huber = 0.0;
}

extern "C" int mv_pg_solve_dev(mv_context *ctx, const mv_pg_params *p, int batch, int nodes, int num_edges, int env_cap,
                               const float *poses_in, const int *edge_offsets, const int *edge_i, const int *edge_j,
                               const int *edge_kind, const float *edge_z, const float *edge_w, const int *node_fixed,
                               float *poses_out, double *cost_initial, double *cost_final, int *iters, int *status) {
    MV_REQUIRE(ctx && p && batch > 0 && nodes >= 2 && nodes <= MV_PG_MAX_NODES && env_cap >= 1);
    MV_REQUIRE(num_edges >= 0 && poses_in && edge_offsets && poses_out);
    MV_REQUIRE(num_edges == 0 || (edge_i && edge_j && edge_kind && edge_z && edge_w));
    MV_REQUIRE(cost_initial && cost_final && iters && status);
    MV_REQUIRE(mv::lm_params_ok(*p, p->huber));
    MV_REQUIRE((long)batch * nodes < (1l << 31));
    const size_t lds = (size_t)12 * nodes * sizeof(double) + (size_t)(5 * nodes + 2) * sizeof(int);  // 58 KiB at 512
    MV_HIP_TRY(hipSetDevice(ctx->device));
    // no envelope is larger than the full lower triangle
    const size_t ecap = (size_t)std::max(num_edges, 1);
    const size_t envc = (size_t)std::min<long>(env_cap, (long)nodes * (nodes + 1) / 2);
    const size_t slab = mv::carve_bytes(pg_scratch_layout, (size_t)2, ecap, envc, (size_t)nodes) -
                        mv::carve_bytes(pg_scratch_layout, (size_t)1, ecap, envc, (size_t)nodes);  // of one workgroup
    const int grid = mv::solver_grid(ctx, batch, slab, "MV_PG_GRID");
    PgScratch m;
    if (!mv::carve(mv::scratch, ctx, [&](mv::Carve &c) { m = pg_scratch_layout(c, (size_t)grid, ecap, envc, (size_t)nodes); }))
        return MV_ERR_OUT_OF_MEMORY;
    MV_LAUNCH("k_pg_solve", k_pg_solve, dim3((unsigned)grid), dim3(NT), lds, ctx->stream, *p, batch, nodes, num_edges,
              env_cap, poses_in, edge_offsets, edge_i, edge_j, edge_kind, edge_z, edge_w, node_fixed,
              poses_out, cost_initial, cost_final, iters, status, m, (int)envc);
    return mv::set_status(MV_OK);
}

extern "C" int mv_pg_edges_from_transforms_dev(mv_context *ctx, int E, const float *T12, float *z7) {
    MV_REQUIRE(ctx && E >= 0 && (E == 0 || (T12 && z7)));
    if (E == 0) return mv::set_status(MV_OK);
    MV_HIP_TRY(hipSetDevice(ctx->device));
    MV_LAUNCH("k_pg_edges_from_transforms", k_pg_edges_from_transforms, dim3((unsigned)((E + 255) / 256)), dim3(256), 0,
              ctx->stream, E, T12, z7);
    return mv::set_status(MV_OK);
}
