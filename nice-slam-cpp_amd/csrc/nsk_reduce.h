// nsk_reduce.h -- the reductions the evaluation kernels share: the wave butterfly, the tail of a "partial rows" kernel with the kernel that
// finishes the rows, and the workgroup scan.
//
// The association of a row reduction is a contract (include/nsk.h promises "two runs, the same bytes"; tests/rows_checks.py restates the
// tree in numpy and tests/test_gpu_rows.py holds the device to it bytes for bytes):
//   - a lane combines its elements in index order over a grid-stride loop, starting from +0.0;
//   - the 64 lanes of a wave meet by xor shuffles, v = v o v[lane ^ s] for s = 32, 16, 8, 4, 2, 1 (wave_all);
//   - the four waves of the workgroup meet through LDS in wave order, ((w0 o w1) o w2) o w3, and the workgroup writes one row (rows_store);
//   - k_rows_finish combines the rows in index order: a sum from +0.0, a minimum / maximum from the first row;
//   - the grid is a function of the element count alone (rows_reduce in nsk.hip: min(ceil(n / 256), cap) rows).
// No floating-point atomics anywhere.  Rows are doubles throughout: a float widens exactly, and a count is a sum of exact integers.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) < __builtin_inff(); }       // false for NaN and +-inf

// every lane gets the combination of the wave's 64 values; `combine` must be associative and commutative (a sum, a minimum, a maximum, the
// nearer of two candidates).  T: any trivially copyable type made of 32-bit words
template <class T, class F>
__device__ __forceinline__ T wave_all(T v, F combine)
{
    static_assert(sizeof(T) % 4 == 0, "wave_all shuffles 32-bit words");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        int w[sizeof(T) / 4];
        __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
        for (unsigned k = 0; k < sizeof(T) / 4; ++k) w[k] = __shfl_xor(w[k], o, 64);
        T other;
        __builtin_memcpy(&other, w, sizeof(T));
        v = combine(v, other);
    }
    return v;
}

// ---- rows ---------------------------------------------------------------------------------------------------------------------------------
// The columns of a row reduction are a type: N columns, op(k) what column k does.
enum RowOp { ROW_SUM, ROW_MIN, ROW_MAX };
template <int COLS> struct RowSums { static constexpr int N = COLS; static constexpr RowOp op(int) { return ROW_SUM; } };
__device__ __forceinline__ double row_combine(RowOp op, double a, double b) { return op == ROW_SUM ? a + b : (op == ROW_MIN ? fmin(a, b) : fmax(a, b)); }

// the tail of a partial-rows kernel (256 threads): the lanes' acc -> row[0 .. N), the row of this workgroup
template <class Cols>
__device__ __forceinline__ void rows_store(const double (&acc)[Cols::N], double* __restrict__ row)
{
    __shared__ double sh[4][Cols::N];
#pragma unroll
    for (int k = 0; k < Cols::N; ++k) {
        const double s = wave_all(acc[k], [k](double a, double b) { return row_combine(Cols::op(k), a, b); });
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < Cols::N) {
        const RowOp op = Cols::op(k);
        row[k] = row_combine(op, row_combine(op, row_combine(op, sh[0][k], sh[1][k]), sh[2][k]), sh[3][k]);
    }
}

// rows: [groups][nrows][N]; thread (group, k) combines column k of its group's rows in index order -> out[group * N + k]
template <class Cols>
__global__ __launch_bounds__(256) void k_rows_finish(int groups, int nrows, const double* __restrict__ rows, double* __restrict__ out)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)groups * Cols::N) return;
    const int k = (int)(g % Cols::N);
    const RowOp op = Cols::op(k);
    const double* col = rows + (size_t)(g / Cols::N) * nrows * Cols::N + k;
    double s = op == ROW_SUM ? 0.0 : col[0];
    for (int r = op == ROW_SUM ? 0 : 1; r < nrows; ++r) s = row_combine(op, s, col[(size_t)r * Cols::N]);
    out[g] = s;
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------------------
// inclusive scan of one value per thread over the 256 threads of a workgroup (lanes by shuffles, the four waves in wave order); *total =
// the workgroup's sum.  (An exclusive scan: the result minus the thread's own value.)
template <class T>
__device__ __forceinline__ T block_scan(T v, T* total)
{
    __shared__ T wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    __syncthreads();                        // (a second scan in the same kernel must not overtake the readers of the first)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    T base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    *total = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    return base + inc;
}
