// ViM open-set scores (Wang, Li, Feng, Zhang, "ViM: Out-Of-Distribution with Virtual-logit Matching", CVPR 2022) on the GPU, and the
// symmetric eigensolver they need. include/osi.h (ABI 26) is the definition; openset_imagenet/vim.py is the user's face of it.
//
//   eigh      parallel cyclic Jacobi in fp64 under the round-robin ordering: a sweep is n - 1 rounds (n = F rounded up to even), a round
//             n / 2 disjoint pairs that are a function of (F, round) alone. A round is two launches. k_eigh_angles (one workgroup) reads
//             a_pp, a_qq, a_pq of every pair from the matrix as the previous round left it and writes, per COLUMN j, the two
//             coefficients of out_j = cc[j] in_j + ss[j] in_partner(j); an unrotated pair and the bye column of an odd F get (1, 0).
//             k_eigh_rotate runs one workgroup per pair: rows p and q come into LDS with coalesced loads and are rotated on the way
//             (J^T A), then every column rotation of the round is applied inside those two rows from LDS (A J) and the rows are stored,
//             coalesced. No workgroup touches another's rows and nothing walks a column through global memory. The rows p and q of Vt
//             are rotated by the same workgroup. The count of rotations is an integer sum of one workgroup; no atomics anywhere.
//   project   z = (x - origin) R^T on gemm_tile (gemm_f64.h), the subtraction one rounded fp64 operation in the operand loader.
//   scores    one wave per row: the norm of z, the logsumexp of the logits and the softmax with the virtual logit, fixed-order sums.
// Addressing is 64-bit throughout; the argument checks keep every element count below 2^31 (include/osi.h).
#include "gemm_f64.h"

#include <math.h>

namespace {

constexpr int MAX_F = OSI_EIGH_MAX_F;
constexpr size_t WS_HEAD = 64;              // bytes every call asks for
constexpr int NORM_BLOCKS = 1024;           // most partial sums of the Frobenius norm
static_assert(2 * MAX_F * sizeof(double) <= 65536, "two rows of the widest matrix fit the LDS of one workgroup");

// ---- the round-robin ordering: n players (n even), n - 1 rounds; player n - 1 stays, the others turn. Pair m of round r -------------
__device__ __forceinline__ void pair_of(int n, int r, int m, int& p, int& q) {
    const int n1 = n - 1;
    int a = n1, b = r;
    if (m > 0) {
        a = r + m;
        a = a >= n1 ? a - n1 : a;
        b = r - m;
        b = b < 0 ? b + n1 : b;
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}
__device__ __forceinline__ int partner_of(int n, int r, int j) {
    const int n1 = n - 1;
    if (j == n1) return r;
    if (j == r) return n1;
    int k = 2 * r - j;                      // in (-n1, 2 n1)
    k = k < 0 ? k + n1 : k;
    return k >= n1 ? k - n1 : k;
}

// -------------------------------------------------------------------------------------------------------------------- begin
__global__ __launch_bounds__(NT) void k_eigh_init(const double* __restrict__ S, int F, double* __restrict__ A, double* __restrict__ Vt,
                                                 double* __restrict__ part) {
    __shared__ double sh[NT];
    const size_t total = (size_t)F * (size_t)F;
    double s = 0.0;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const double v = S[e];
        const size_t i = e / (size_t)F;
        A[e] = v;
        Vt[e] = e - i * (size_t)F == i ? 1.0 : 0.0;
        s = fma(v, v, s);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(NT) void k_eigh_norm(const double* __restrict__ part, int nparts, double* __restrict__ head,
                                                 int* __restrict__ info) {
    __shared__ double sh[NT];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += NT) s += part[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s);
        head[0] = norm;
        head[1] = norm * 0x1p-52;
        info[0] = (norm - norm == 0.0) ? 0 : 1;             // Inf and NaN fail the test
    }
}

// -------------------------------------------------------------------------------------------------------------------- sweep
__global__ __launch_bounds__(NT) void k_eigh_angles(const double* __restrict__ A, int F, int n, int r, const double* __restrict__ head,
                                                   const int* __restrict__ info, double* __restrict__ cc, double* __restrict__ ss,
                                                   int* __restrict__ rot, long long* __restrict__ rotations) {
    __shared__ int sh[NT];
    if (info[0] != 0) {                                     // uniform
        if (r == 0 && threadIdx.x == 0) rotations[0] = 0;
        return;
    }
    const double tau = head[1];
    int cnt = 0;
    for (int m = threadIdx.x; m < n / 2; m += NT) {
        int p, q;
        pair_of(n, r, m, p, q);
        if (q >= F) {                                       // the bye of an odd F: column p keeps its values
            cc[p] = 1.0;
            ss[p] = 0.0;
            rot[p] = 0;
            continue;
        }
        const double apq = A[(size_t)p * (size_t)F + (size_t)q];
        double c = 1.0, s = 0.0;
        int rt = 0;
        if (fabs(apq) > tau) {
            const double app = A[(size_t)p * (size_t)F + (size_t)p], aqq = A[(size_t)q * (size_t)F + (size_t)q];
            const double theta = (aqq - app) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
            rt = 1;
            ++cnt;
        }
        cc[p] = c;
        cc[q] = c;
        ss[p] = -s;                                         // column p' = c col_p - s col_q, column q' = c col_q + s col_p
        ss[q] = s;
        rot[p] = rt;
        rot[q] = rt;
    }
    cnt = block_sum(cnt, sh);
    if (threadIdx.x == 0) rotations[0] = (r == 0 ? 0ll : rotations[0]) + (long long)cnt;
}

// one workgroup per pair (p, q) of round r; the pair with the dummy player of an odd F is row p alone (column rotations only)
__global__ __launch_bounds__(NT) void k_eigh_rotate(double* __restrict__ A, double* __restrict__ Vt, int F, int n, int r,
                                                   const double* __restrict__ cc, const double* __restrict__ ss,
                                                   const int* __restrict__ rot, const int* __restrict__ info) {
    extern __shared__ double rows[];                        // [2][F]
    if (info[0] != 0) return;                               // uniform
    int p, q;
    pair_of(n, r, (int)blockIdx.x, p, q);
    const bool two = q < F;                                 // uniform
    double* rp = rows;
    double* rq = rows + F;
    const double c = cc[p], s = -ss[p];
    const bool rotated = rot[p] != 0;
    double* Ap = A + (size_t)p * (size_t)F;
    double* Aq = A + (size_t)(two ? q : p) * (size_t)F;
    for (int j = threadIdx.x; j < F; j += NT) {             // J^T A: the two rows
        const double ap = Ap[j];
        if (two) {
            const double aq = Aq[j];
            rp[j] = c * ap - s * aq;
            rq[j] = s * ap + c * aq;
        } else {
            rp[j] = ap;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < F; j += NT) {             // (J^T A) J: every pair of columns of the round, inside the two rows
        int k = partner_of(n, r, j);
        k = k < F ? k : j;                                  // the bye column: (1, 0)
        const double cj = cc[j], sj = ss[j];
        double vp = cj * rp[j] + sj * rp[k];
        if (rotated && j == q) vp = 0.0;
        Ap[j] = vp;
        if (two) {
            double vq = cj * rq[j] + sj * rq[k];
            if (rotated && j == p) vq = 0.0;
            Aq[j] = vq;
        }
    }
    if (two && rotated) {                                   // J^T Vt; an unrotated pair is (1, 0): the rows keep their bits
        double* Vp = Vt + (size_t)p * (size_t)F;
        double* Vq = Vt + (size_t)q * (size_t)F;
        for (int j = threadIdx.x; j < F; j += NT) {
            const double vp = Vp[j], vq = Vq[j];
            Vp[j] = c * vp - s * vq;
            Vq[j] = s * vp + c * vq;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- finish
// workgroup i: the rank of a_ii among the diagonal (descending, ties by index, a NaN last), then row i of Vt to that row, signed
__global__ __launch_bounds__(NT) void k_eigh_finish(const double* __restrict__ A, const double* __restrict__ Vt, int F,
                                                   const int* __restrict__ info, double* __restrict__ evals, double* __restrict__ evecs) {
    __shared__ int shi[NT];
    __shared__ double shv[NT];
    const int i = blockIdx.x;
    if (info[0] != 0) {                                     // uniform
        if (threadIdx.x == 0) evals[i] = NAN;
        for (int j = threadIdx.x; j < F; j += NT) evecs[(size_t)i * (size_t)F + (size_t)j] = 0.0;
        return;
    }
    const double di = A[(size_t)i * (size_t)F + (size_t)i];
    const bool di_nan = di != di;
    int before = 0;
    for (int j = threadIdx.x; j < F; j += NT) {
        const double dj = A[(size_t)j * (size_t)F + (size_t)j];
        const bool dj_nan = dj != dj;
        const bool b = di_nan ? (!dj_nan || j < i) : (dj > di || (dj == di && j < i));
        before += b ? 1 : 0;
    }
    const int rank = block_sum(before, shi);
    const double* v = Vt + (size_t)i * (size_t)F;
    double best = -1.0;
    int at = 0;
    for (int j = threadIdx.x; j < F; j += NT) {             // ascending j: a strict comparison keeps the first of equals
        const double a = fabs(v[j]);
        if (a > best) {
            best = a;
            at = j;
        }
    }
    shv[threadIdx.x] = best;
    shi[threadIdx.x] = at;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double b2 = shv[threadIdx.x + o];
            const int a2 = shi[threadIdx.x + o];
            if (b2 > shv[threadIdx.x] || (b2 == shv[threadIdx.x] && a2 < shi[threadIdx.x])) {
                shv[threadIdx.x] = b2;
                shi[threadIdx.x] = a2;
            }
        }
        __syncthreads();
    }
    const bool flip = v[shi[0]] < 0.0;
    if (threadIdx.x == 0) evals[rank] = di;
    for (int j = threadIdx.x; j < F; j += NT) evecs[(size_t)rank * (size_t)F + (size_t)j] = flip ? -v[j] : v[j];
}

// ------------------------------------------------------------------------------------------------------------------ project
// K-minor over the rows of x, shifted: (double)x[row][k] - origin[k], one rounded subtraction; the layout of RowsOfMatrix
struct ShiftedRows {
    const float* p;
    const double* origin;
    size_t ld;
    int r0, rows;
    __device__ __forceinline__ void fetch(int k0, int kend, double (&r)[EPT]) const {
        const int k = k0 + (int)(threadIdx.x & 15), ii = (int)(threadIdx.x >> 4);
        const double o = k < kend ? origin[k] : 0.0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int row = r0 + ii + 16 * e;
            r[e] = (row < rows && k < kend) ? __dsub_rn((double)p[(size_t)row * ld + (size_t)k], o) : 0.0;
        }
    }
    __device__ __forceinline__ void put(double (*s)[LDT], const double (&r)[EPT]) const {
        const int k = (int)(threadIdx.x & 15), ii = (int)(threadIdx.x >> 4);
#pragma unroll
        for (int e = 0; e < EPT; ++e) s[k][ii + 16 * e] = r[e];
    }
};

__global__ __launch_bounds__(NT) void k_vim_project(const float* __restrict__ x, const double* __restrict__ origin, int M, int F,
                                                   const double* __restrict__ R, int K, double* __restrict__ z) {
    __shared__ Tile sm;
    const int i0 = (int)blockIdx.x * TM, j0 = (int)blockIdx.y * TM;
    const ShiftedRows la{x, origin, (size_t)F, i0, M};
    const RowsOfMatrix<double> lb{R, (size_t)F, j0, K};
    f64x4 acc[2][2];
    gemm_tile(sm, la, lb, 0, F, acc);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = i0 + tile_i(ti, r), gj = j0 + tile_j(tj);
                if (gi < M && gj < K) z[(size_t)gi * (size_t)K + (size_t)gj] = acc[ti][tj][r];
            }
}

// ------------------------------------------------------------------------------------------------------------------- scores
// the maximum of the logits is taken with wave_fmax: a NaN is skipped there and comes back through the sums
__global__ __launch_bounds__(NT) void k_vim_scores(const double* __restrict__ z, int M, int K, const float* __restrict__ logits, int C,
                                                  double alpha, int mode, float* __restrict__ o32, double* __restrict__ o64) {
    const int lane = threadIdx.x & 63;
    for (long long i = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); i < M; i += (long long)gridDim.x * (NT / 64)) {
        const double* zr = z + (size_t)i * (size_t)K;
        double sq = 0.0;
        for (int k = lane; k < K; k += 64) sq = fma(zr[k], zr[k], sq);
        const double norm = sqrt(wave_sum(sq));
        if (mode == OSI_VIM_NORM) {
            if (lane == 0) {
                if (o32) o32[i] = (float)norm;
                else o64[i] = norm;
            }
            continue;
        }
        const double v = alpha * norm;                      // the virtual logit
        const float* lr = logits + (size_t)i * (size_t)C;
        double mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmax(mx, (double)lr[c]);
        mx = wave_fmax(mx);
        if (mode == OSI_VIM_PROBS) mx = fmax(mx, v);
        const double shift = (mx - mx == 0.0) ? mx : 0.0;   // an infinite maximum is not subtracted
        double se = 0.0;
        for (int c = lane; c < C; c += 64) se += exp((double)lr[c] - shift);
        se = wave_sum(se);
        if (mode == OSI_VIM_UNKNOWN) {
            const double u = v - (shift + log(se));
            if (lane == 0) {
                if (o32) o32[i] = (float)u;
                else o64[i] = u;
            }
            continue;
        }
        const double ev = exp(v - shift), denom = se + ev;
        const size_t o = (size_t)i * (size_t)(C + 1);
        for (int c = lane; c <= C; c += 64) {
            const double pr = (c < C ? exp((double)lr[c] - shift) : ev) / denom;
            if (o32) o32[o + (size_t)c] = (float)pr;
            else o64[o + (size_t)c] = pr;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------- host
inline int tiles_of(int n) { return (n + TM - 1) / TM; }
inline size_t eigh_ws(int F) { return WS_HEAD + ((size_t)NORM_BLOCKS + 2 * (size_t)F) * 8 + ((size_t)F * 4 + 7) / 8 * 8; }
inline bool ws_ok(const void* ws, size_t have, size_t need) { return ws && have >= need && ((uintptr_t)ws & 7) == 0; }
inline int norm_blocks(int F) {                             // a function of F alone: the summation order is part of the result
    const size_t b = ((size_t)F * (size_t)F + NT - 1) / NT;
    return (int)(b < (size_t)NORM_BLOCKS ? b : (size_t)NORM_BLOCKS);
}
struct EighWs {
    double *part, *cc, *ss;
    int* rot;
    EighWs(void* ws, int F) {
        part = reinterpret_cast<double*>(static_cast<char*>(ws) + WS_HEAD);
        cc = part + NORM_BLOCKS;
        ss = cc + F;
        rot = reinterpret_cast<int*>(ss + F);
    }
};

}  // namespace

extern "C" {

size_t osi_vim_workspace(int M, int K, int F) {
    if (M <= 0 || K <= 0 || F <= 0 || F > MAX_F || K > MAX_F) return 0;
    return eigh_ws(F);
}

int osi_eigh_begin(const double* S, int F, double* A, double* Vt, double* head, int* info, void* ws, size_t ws_bytes,
                   osi_stream_t stream) {
    OSI_REQUIRE(S && A && Vt && head && info);
    OSI_REQUIRE(F > 0 && F <= MAX_F);
    OSI_REQUIRE(ws_ok(ws, ws_bytes, eigh_ws(F)));
    const EighWs w(ws, F);
    const int nb = norm_blocks(F);
    hipLaunchKernelGGL(k_eigh_init, dim3(nb), dim3(NT), 0, (hipStream_t)stream, S, F, A, Vt, w.part);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_eigh_norm, dim3(1), dim3(NT), 0, (hipStream_t)stream, w.part, nb, head, info);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_eigh_sweep(double* A, double* Vt, int F, const double* head, const int* info, long long* rotations, void* ws, size_t ws_bytes,
                   osi_stream_t stream) {
    OSI_REQUIRE(A && Vt && head && info && rotations);
    OSI_REQUIRE(F > 0 && F <= MAX_F);
    OSI_REQUIRE(ws_ok(ws, ws_bytes, eigh_ws(F)));
    const EighWs w(ws, F);
    const int n = (F + 1) / 2 * 2;
    const size_t lds = 2 * (size_t)F * sizeof(double);
    for (int r = 0; r < n - 1; ++r) {
        hipLaunchKernelGGL(k_eigh_angles, dim3(1), dim3(NT), 0, (hipStream_t)stream, A, F, n, r, head, info, w.cc, w.ss, w.rot, rotations);
        OSI_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_eigh_rotate, dim3(n / 2), dim3(NT), lds, (hipStream_t)stream, A, Vt, F, n, r, w.cc, w.ss, w.rot, info);
        OSI_LAUNCH_CHECK();
    }
    return OSI_OK;
}

int osi_eigh_finish(const double* A, const double* Vt, int F, const int* info, double* evals, double* evecs, void* ws, size_t ws_bytes,
                    osi_stream_t stream) {
    OSI_REQUIRE(A && Vt && info && evals && evecs);
    OSI_REQUIRE(F > 0 && F <= MAX_F);
    OSI_REQUIRE(ws_ok(ws, ws_bytes, eigh_ws(F)));
    hipLaunchKernelGGL(k_eigh_finish, dim3(F), dim3(NT), 0, (hipStream_t)stream, A, Vt, F, info, evals, evecs);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_vim_project_f32(const float* x, const double* origin, int M, int F, const double* R, int K, double* z, void* ws, size_t ws_bytes,
                        osi_stream_t stream) {
    OSI_REQUIRE(x && origin && R && z);
    OSI_REQUIRE(M > 0 && F > 0 && K > 0 && F <= MAX_F && K <= MAX_F);
    OSI_REQUIRE((long long)M * F < MAX_ELEMS && (long long)M * K < MAX_ELEMS);
    OSI_REQUIRE(ws_ok(ws, ws_bytes, WS_HEAD));
    hipLaunchKernelGGL(k_vim_project, dim3(tiles_of(M), tiles_of(K)), dim3(NT), 0, (hipStream_t)stream, x, origin, M, F, R, K, z);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_vim_scores(const double* z, int M, int K, const float* logits, int C, double alpha, int mode, float* out_f32, double* out_f64,
                   void* ws, size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(z);
    OSI_REQUIRE((out_f32 != nullptr) != (out_f64 != nullptr));
    OSI_REQUIRE(mode == OSI_VIM_NORM || mode == OSI_VIM_UNKNOWN || mode == OSI_VIM_PROBS);
    OSI_REQUIRE(M > 0 && K > 0 && K <= MAX_F && (long long)M * K < MAX_ELEMS);
    if (mode != OSI_VIM_NORM) {
        OSI_REQUIRE(logits && C > 0 && (long long)M * ((long long)C + 1) < MAX_ELEMS);
        OSI_REQUIRE(alpha - alpha == 0.0);                  // finite
    }
    OSI_REQUIRE(ws_ok(ws, ws_bytes, WS_HEAD));
    const long long blocks = ((long long)M + NT / 64 - 1) / (NT / 64);
    hipLaunchKernelGGL(k_vim_scores, dim3((int)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(NT), 0, (hipStream_t)stream, z, M, K,
                       logits, C, alpha, mode, out_f32, out_f64);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
