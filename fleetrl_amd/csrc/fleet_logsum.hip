// fleet_logsum.hip -- the data-log ring reduced to the evaluation's numbers on the device (fleet_log_summary_dev; the reference's
// agent_eval/basic_evaluation.py sums the DataLogger frames on the host).  DESIGN.md "The data log, summarised on the device".
//
// Two launches, no atomics, one fixed order of additions (so the result does not depend on the launch geometry and
// tests/logsum_model.py restates it bit for bit):
//   logsum_partial   one wavefront per (env, block of 64 window rows).  The rows' scalars are read with row r in lane r and summed
//                    through lane reads in ascending r; the rows' EVs are walked oldest row first, one EV per lane and the EVs in
//                    chunks of 64.  Every accumulator starts at +0.0 and takes its rows in ascending order.  Leaves the block's
//                    partials in the handle's scratch: 8 scalars, N degradation sums, 64 (row power, time-of-day slot) pairs and
//                    the block's histogram.
//   logsum_fold      one workgroup per env: adds the block partials in ascending block order and writes the outputs.
// Everything is float64 and compiled without contraction (build.py: -ffp-contract=off).
#include "fleet_logsum.h"

namespace {

struct LogsumScratch {
  double* scal;      // [E,nb,8]
  double* deg;       // [E,nb,N]
  double* row_pow;   // [E,nb,64]
  int32_t* row_slot; // [E,nb,64]
  int32_t* hist;     // [E,nb,256]
  int nb;            // blocks of a full ring
};

__host__ __device__ inline LogsumScratch logsum_carve(void* base, int E, int N, int log_cap) {
  LogsumScratch s;
  s.nb = (log_cap + kLogsumRows - 1) / kLogsumRows;
  const size_t eb = (size_t)E * s.nb;
  s.scal = static_cast<double*>(base);
  s.deg = s.scal + eb * 8;
  s.row_pow = s.deg + eb * (size_t)N;
  s.row_slot = reinterpret_cast<int32_t*>(s.row_pow + eb * kLogsumRows);
  s.hist = s.row_slot + eb * kLogsumRows;
  return s;
}

// what the kernels read of the handle: the ring and its sizes
struct LogsumRing {
  int E, N, T, cap;
  const int32_t* pos;
  const int32_t* row;
  const double* env;
  const double* ev;
};

// the kept rows k0 <= k < k0 + W of env e, oldest first; row k lies in slot k % cap
__device__ __forceinline__ void logsum_window(const LogsumRing& g, int drop_last, int e, long long* k0, int* W) {
  const long long pos = g.pos[e];
  const long long lo = pos > g.cap ? pos - g.cap : 0;
  const long long hi = pos - drop_last > lo ? pos - drop_last : lo;
  *k0 = lo;
  *W = (int)(hi - lo);
}

__device__ __forceinline__ double hist_edge(double lo, double hi, double step, int bins, int i) {
  return i >= bins ? hi : lo + (double)i * step;
}

// the value lane `l` holds (l the same in every lane)
__device__ __forceinline__ double lane_value(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__global__ __launch_bounds__(kLogsumRows) void logsum_partial(LogsumRing g, FleetLogsumArgs a) {
  const int e = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  long long k0;
  int W;
  logsum_window(g, a.drop_last, e, &k0, &W);
  const int jbeg = b * kLogsumRows;
  if (e >= g.E || jbeg >= W) return;  // (uniform: a block past the env's window leaves no partial, the fold reads none)
  const int rows = W - jbeg < kLogsumRows ? W - jbeg : kLogsumRows;
  const LogsumScratch sc = logsum_carve(a.scratch, g.E, g.N, g.cap);
  const size_t blk = (size_t)e * sc.nb + b;
  const int N = g.N, nch = (N + 63) / 64;
  const bool want_prof = a.minutes_per_step > 0 && (a.prof_sum || a.prof_cnt);
  const bool want_hist = a.hist != nullptr;

  __shared__ int32_t h[kLogsumMaxBins];
  if (want_hist) {
    for (int i = lane; i < kLogsumMaxBins; i += 64) h[i] = 0;
    __syncthreads();
  }
  const double step = (a.hi - a.lo) / (double)a.bins;
  const double per_step = 1.0 / step;  // for the first guess of a bin only: the walk along the edges decides
  const unsigned long long le_mask = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);  // lanes <= this one

  // ---- the rows' scalars: row r in lane r, one round trip for the whole block ---------------------------------------------------
  const bool has = lane < rows;
  const size_t my_base = (size_t)(int)((k0 + jbeg + (has ? lane : 0)) % g.cap) * g.E + e;
  const uint32_t raw = has ? (uint32_t)g.row[my_base] : 0u;
  const bool my_reset = (raw >> 31) != 0;
  const int t = (int)(raw & 0x7FFFFFFFu);
  const int hm = (has && t < g.T) ? (a.tab_hm[t] & 0x7FFF) : 0;  // hour << 8 | minute
  const double* le = g.env + my_base * 4;
  const double rew = has ? le[0] : 0.0, cash = has ? le[1] : 0.0;
  const double over = has ? fabs(le[2]) : 0.0, socv = has ? fabs(le[3]) : 0.0;
  const double cpm = cash * a.price_multiplier;
  const double pen = my_reset ? 0.0 : rew - cpm;
  const unsigned long long reset_rows = __ballot(has && my_reset);
  // bit r: row r of the block is a degradation row
  const unsigned long long deg_rows = __ballot(has && !my_reset && a.calc_deg && hm == ((14 << 8) | 45));
  const int n_viol = __popcll(__ballot(has && socv > 0.0)), n_deg = __popcll(deg_rows);
  const int my_slot = (60 * (hm >> 8) + (hm & 0xFF)) / (a.minutes_per_step > 0 ? a.minutes_per_step : 1);
  double s_rew = 0.0, s_cash = 0.0, s_pen = 0.0, s_over = 0.0, s_socv = 0.0;
  for (int r = 0; r < rows; ++r) {  // ascending rows: every lane adds the same values in the same order
    s_rew += lane_value(rew, r);
    s_cash += lane_value(cash, r);
    s_pen += lane_value(pen, r);
    s_over += lane_value(over, r);
    s_socv += lane_value(socv, r);
  }

  // ---- the rows' EVs: one EV per lane, chunks of 64; the first chunk of the next row is on its way while this row is folded -----
  double my_pow = 0.0;  // lane r keeps row r's power
  if (want_prof || want_hist) {
    const bool ok0 = lane < N;
    const double* ev_next = g.ev + ((size_t)(int)((k0 + jbeg) % g.cap) * g.E + e) * 4 * (size_t)N;
    double act_next = ok0 ? ev_next[lane] : 0.0, en_next = (ok0 && want_prof) ? ev_next[N + lane] : 0.0;
    for (int r = 0; r < rows; ++r) {
      const bool reset = ((reset_rows >> r) & 1ull) != 0;
      const double* ev = ev_next;
      const double act0 = act_next, en0 = en_next;
      if (r + 1 < rows) {
        ev_next = g.ev + ((size_t)(int)((k0 + jbeg + r + 1) % g.cap) * g.E + e) * 4 * (size_t)N;
        act_next = ok0 ? ev_next[lane] : 0.0;
        en_next = (ok0 && want_prof) ? ev_next[N + lane] : 0.0;
      }
      double carry_c = 0.0, carry_d = 0.0, row_sum = 0.0;  // Q8: the last charging / discharging energy of the chunks so far
      for (int ch = 0; ch < nch; ++ch) {
        const int c = ch * 64 + lane;
        const bool ok = c < N;
        const double act = ch == 0 ? act0 : (ok ? ev[c] : 0.0);
        if (want_prof) {
          const double en = ch == 0 ? en0 : (ok ? ev[N + c] : 0.0);
          const unsigned long long pc = __ballot(ok && act >= 0.0), pd = __ballot(ok && act < 0.0);
          const unsigned long long mc = pc & le_mask, md = pd & le_mask;
          const double ec = __shfl(en, mc ? 63 - __clzll((long long)mc) : lane);
          const double ed = __shfl(en, md ? 63 - __clzll((long long)md) : lane);
          const double ce = mc ? ec : carry_c, de = md ? ed : carry_d;
          double v = (ok && !reset) ? ce + de : 0.0;
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
          row_sum += v;
          if (pc) carry_c = lane_value(en, 63 - __clzll((long long)pc));
          if (pd) carry_d = lane_value(en, 63 - __clzll((long long)pd));
        }
        if (want_hist) {
          int bin = -1;
          if (ok && (a.hist_ev < 0 || c == a.hist_ev) && act >= a.lo && act <= a.hi) {  // (NaN: not counted)
            const double f = (act - a.lo) * per_step;
            int i = f >= (double)(a.bins - 1) ? a.bins - 1 : (f > 0.0 ? (int)f : 0);
            while (i > 0 && act < hist_edge(a.lo, a.hi, step, a.bins, i)) --i;
            while (i < a.bins - 1 && act >= hist_edge(a.lo, a.hi, step, a.bins, i + 1)) ++i;
            bin = i;
          }
          // one pass per distinct bin among the lanes; lane 0 alone touches the block's histogram
          unsigned long long todo = __ballot(bin >= 0);
          while (todo) {
            const int bb = __builtin_amdgcn_readlane(bin, __ffsll((long long)todo) - 1);
            const unsigned long long m = __ballot(bin == bb);
            if (lane == 0) h[bb] += __popcll(m);
            todo &= ~m;
          }
        }
      }
      if (lane == r) my_pow = row_sum;
    }
    my_pow = my_pow / (double)N;  // (row r's EV sum in lane r: one division for the block's rows)
  }

  if (lane == 0) {
    double* p = sc.scal + blk * 8;
    p[0] = (double)rows;
    p[1] = s_rew;
    p[2] = s_cash;
    p[3] = s_pen;
    p[4] = s_over;
    p[5] = s_socv;
    p[6] = (double)n_viol;
    p[7] = (double)n_deg;
  }
  if (want_prof && lane < rows) {
    sc.row_pow[blk * kLogsumRows + lane] = my_pow;
    sc.row_slot[blk * kLogsumRows + lane] = my_slot;
  }
  if (want_hist) {
    __syncthreads();
    for (int i = lane; i < a.bins; i += 64) sc.hist[blk * kLogsumMaxBins + i] = h[i];
  }
  if (a.deg_sum) {  // the degradation rows only (one per day): every other row adds +0.0, which changes no sum that began at +0.0
    for (int ch = 0; ch < nch; ++ch) {
      const int c = ch * 64 + lane;
      if (c >= N) break;
      double acc = 0.0;
      for (unsigned long long m = deg_rows; m; m &= m - 1) {
        const int r = __ffsll((long long)m) - 1;
        const int slot = (int)((k0 + jbeg + r) % g.cap);
        acc += g.ev[(((size_t)slot * g.E + e) * 4 + 2) * (size_t)N + c];
      }
      sc.deg[blk * (size_t)N + c] = acc;
    }
  }
}

__global__ __launch_bounds__(kLogsumFoldThreads) void logsum_fold(LogsumRing g, FleetLogsumArgs a) {
  const int e = blockIdx.x, tid = threadIdx.x;
  if (e >= g.E) return;
  long long k0;
  int W;
  logsum_window(g, a.drop_last, e, &k0, &W);
  const LogsumScratch sc = logsum_carve(a.scratch, g.E, g.N, g.cap);
  const int nb = (W + kLogsumRows - 1) / kLogsumRows, N = g.N;
  const size_t blk0 = (size_t)e * sc.nb;

  if (tid < 8) {
    double tot = 0.0;
    if (tid == 0) tot = (double)W;
    else
      for (int b = 0; b < nb; ++b) tot += sc.scal[(blk0 + b) * 8 + tid];
    a.scal[(size_t)e * 8 + tid] = tot;
  }
  if (a.deg_sum)
    for (int c = tid; c < N; c += kLogsumFoldThreads) {
      double tot = 0.0;
      for (int b = 0; b < nb; ++b) tot += sc.deg[(blk0 + b) * (size_t)N + c];
      a.deg_sum[(size_t)e * N + c] = tot;
    }
  if (a.soh_last) {
    const int slot = W > 0 ? (int)((k0 + W - 1) % g.cap) : 0;
    for (int c = tid; c < N; c += kLogsumFoldThreads)
      a.soh_last[(size_t)e * N + c] = W > 0 ? g.ev[(((size_t)slot * g.E + e) * 4 + 3) * (size_t)N + c] : __builtin_nan("");
  }
  if (a.minutes_per_step > 0 && (a.prof_sum || a.prof_cnt)) {
    const int S = 1440 / a.minutes_per_step;
    for (int s = tid; s < S; s += kLogsumFoldThreads) {
      double tot = 0.0;
      int cnt = 0;
      for (int b = 0; b < nb; ++b) {
        const int rows = W - b * kLogsumRows < kLogsumRows ? W - b * kLogsumRows : kLogsumRows;
        const double* pw = sc.row_pow + (blk0 + b) * kLogsumRows;
        const int32_t* sl = sc.row_slot + (blk0 + b) * kLogsumRows;
        double part = 0.0;
        for (int r = 0; r < rows; ++r)
          if (sl[r] == s) {
            part += pw[r];
            cnt += 1;
          }
        tot += part;
      }
      if (a.prof_sum) a.prof_sum[(size_t)e * S + s] = tot;
      if (a.prof_cnt) a.prof_cnt[(size_t)e * S + s] = cnt;
    }
  }
  if (a.hist)
    for (int i = tid; i < a.bins; i += kLogsumFoldThreads) {
      int32_t tot = 0;
      for (int b = 0; b < nb; ++b) tot += sc.hist[(blk0 + b) * kLogsumMaxBins + i];
      a.hist[(size_t)e * a.bins + i] = tot;
    }
}

}  // namespace

size_t fleet_logsum_scratch_bytes(int E, int N, int log_cap) {
  const size_t eb = (size_t)E * ((log_cap + kLogsumRows - 1) / kLogsumRows);
  return eb * ((8 + (size_t)N + kLogsumRows) * sizeof(double) + (kLogsumRows + kLogsumMaxBins) * sizeof(int32_t));
}

hipError_t fleet_launch_log_summary(const FleetDev& d, const FleetLogsumArgs& a, hipStream_t s) {
  const LogsumRing g{d.E, d.N, d.T, d.log_cap, d.log_pos, d.log_row, d.log_env, d.log_ev};
  const unsigned nb = (unsigned)((d.log_cap + kLogsumRows - 1) / kLogsumRows);
  hipLaunchKernelGGL(logsum_partial, dim3((unsigned)d.E, nb), dim3(kLogsumRows), 0, s, g, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(logsum_fold, dim3((unsigned)d.E), dim3(kLogsumFoldThreads), 0, s, g, a);
  return hipGetLastError();
}
