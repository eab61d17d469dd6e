// Traces to miniSEED 2 (volpick_hip.h: vp_mseed_encode): the Steim-1/2 compressor and the plain encodings on the device,
// the 64-byte headers on the host (mseed_write_host.h).  Stands where the reference calls
// waveforms.write(path, format="MSEED") (volpick/data/data.py:1353); ObsPy packs with libmseed on the host.
//
// Steim packing is a chain through the trace: which differences share a word depends on where the previous word ended.
// But word boundaries depend on the trace alone, not on records, and a word takes 1..7 differences, so a chain can enter a
// stretch of samples at only 7 offsets (4 under Steim-1).  Five kernels:
//   classify  one thread per sample: how many differences a word that starts here takes (one byte), out-of-range flagged
//   maps      one wave per chunk of VP_MSEED_ENCODE_CHUNK samples: per entry offset the exit offset and the words used
//             (56 lanes walk 8 sub-chunks x 7 entries in LDS, 7 lanes compose the 8 sub-maps)
//   compose   one wave per trace: each lane composes a run of chunk maps, one lane chains the 64 runs, each lane walks
//             its run again from its true entry -> every chunk's entry offset and first word
//   emit      one wave per chunk: the sub-maps again, then 8 lanes walk the sub-chunks from their true entries and store
//             the first sample of every word at the word's index
//   pack      one thread per 32-bit word of every record's data section: data words, X0, Xn, control words (an OR over
//             the 16 lanes of a frame), zeros behind the end; the thread of X0 also writes the record table
// A record is every 15 * frames - 2 consecutive words of the chain.  No atomics touch the payload; the one atomic is the
// minimum that names the first out-of-range sample.
#include <algorithm>

#include "device_scratch.h"
#include "mseed_write_host.h"

namespace vp {
namespace {

constexpr int L = VP_MSEED_ENCODE_CHUNK;
constexpr int SUB = 256, NSUB = L / SUB;  // sub-chunks a wave walks side by side
constexpr int ENTRIES = 7;                // offsets at which a chain can enter (Steim-1 uses 0..3)
constexpr int CLASSIFY_BLOCK = 256;
static_assert(L % SUB == 0 && NSUB * ENTRIES <= 64 && L % CLASSIFY_BLOCK == 0 && L % 16 == 0, "one wave per chunk");

struct EncTrace {
  long long first;   // where the trace begins in the samples, in elements
  long long n;       // samples
  long long chunk0;  // its first chunk; its classes and word starts begin at chunk0 * L
  long long rec0;    // its first record in the output
};

// the trace that owns chunk / record `v`: the last one whose first chunk / record is not beyond it
template <bool BY_RECORD>
__device__ __forceinline__ int owner(const EncTrace* __restrict__ tr, const int nt, const long long v) {
  int lo = 0, hi = nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((BY_RECORD ? tr[mid].rec0 : tr[mid].chunk0) <= v) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int bits_of(const int d) { return 32 - __builtin_clrsb(d); }  // two's complement width

// cls[chunk0 * L + i]: differences in the word that would start at sample i of the trace; 0 behind the trace's end
template <int VERSION>
__global__ __launch_bounds__(CLASSIFY_BLOCK) void steim_classify_kernel(const int* __restrict__ x,
                                                                        const EncTrace* __restrict__ tr, const int nt,
                                                                        uint8_t* __restrict__ cls,
                                                                        unsigned long long* __restrict__ bad) {
  constexpr int PER = L / CLASSIFY_BLOCK;
  const long long c = blockIdx.x / PER;
  const int t = owner<false>(tr, nt, c);
  const EncTrace T = tr[t];
  const int in_chunk = (int)(blockIdx.x % PER) * CLASSIFY_BLOCK + threadIdx.x;
  const long long i = (c - T.chunk0) * L + in_chunk;
  int cnt = 0;
  if (i < T.n) {
    const int* p = x + T.first + i;
    const long long rem = T.n - i;
    int prev = i > 0 ? p[-1] : 0;
    int m[7];  // m[j]: bits the differences i .. i + j need; 99 once one lies behind the end
    int run = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      int nb = 99;
      if (j < rem) {
        const int cur = p[j];
        nb = bits_of((int)((unsigned)cur - (unsigned)prev));
        prev = cur;
        if (j == 0) {
          if (VERSION == 2 && nb > 30) {
            if (i == 0) nb = 1;  // stored as 0: no decoder reads a trace's first difference
            else atomicMin(bad, ((unsigned long long)t << 40) | (unsigned long long)i);
          }
        }
      }
      run = nb > run ? nb : run;
      m[j] = run;
    }
    if (VERSION == 2)
      cnt = m[6] <= 4 ? 7 : m[5] <= 5 ? 6 : m[4] <= 6 ? 5 : m[3] <= 8 ? 4 : m[2] <= 10 ? 3 : m[1] <= 15 ? 2 : 1;
    else
      cnt = m[3] <= 8 ? 4 : m[1] <= 16 ? 2 : 1;
  }
  cls[c * L + in_chunk] = (uint8_t)cnt;
}

__device__ __forceinline__ void load_classes(const uint8_t* __restrict__ cls, const long long c, uint8_t* s, const int lane) {
  const uint4* g = reinterpret_cast<const uint4*>(cls + c * L);
  uint4* d = reinterpret_cast<uint4*>(s);
  for (int k = lane; k < L / 16; k += 64) d[k] = g[k];
}

// the chain that enters sub-chunk `sub` at offset e: exit offset into the next sub-chunk | words << 3
__device__ __forceinline__ unsigned walk_sub(const uint8_t* s, const int sub, const int e) {
  int pos = sub * SUB + e, w = 0;
  const int end = (sub + 1) * SUB;
  while (pos < end) {
    const int k = s[pos];
    if (k == 0) break;  // the trace ends here
    pos += k;
    ++w;
  }
  return (unsigned)(pos >= end ? pos - end : 0) | ((unsigned)w << 3);
}

// maps[c * 8 + e]: the chain that enters chunk c at offset e leaves it at offset (v & 7) after (v >> 3) words
__global__ __launch_bounds__(64) void steim_maps_kernel(const uint8_t* __restrict__ cls, unsigned* __restrict__ maps) {
  __shared__ __attribute__((aligned(16))) uint8_t s[L];
  __shared__ unsigned sm[NSUB][8];
  const int lane = threadIdx.x;
  const long long c = blockIdx.x;
  load_classes(cls, c, s, lane);
  __syncthreads();
  if (lane < NSUB * ENTRIES) sm[lane / ENTRIES][lane % ENTRIES] = walk_sub(s, lane / ENTRIES, lane % ENTRIES);
  __syncthreads();
  if (lane < ENTRIES) {
    unsigned off = lane, w = 0;
    for (int k = 0; k < NSUB; ++k) {
      const unsigned v = sm[k][off];
      w += v >> 3;
      off = v & 7;
    }
    maps[c * 8 + lane] = off | (w << 3);
  }
}

// cstate[chunk] = (entry offset, first word) of every chunk of trace blockIdx.x; words[trace] = words of the trace
__global__ __launch_bounds__(64) void steim_compose_kernel(const EncTrace* __restrict__ tr, const unsigned* __restrict__ maps,
                                                           int2* __restrict__ cstate, long long* __restrict__ words) {
  __shared__ int run_off[64][ENTRIES], run_words[64][ENTRIES], run_entry[64], run_base[64];
  const int lane = threadIdx.x;
  const EncTrace T = tr[blockIdx.x];
  const long long nchunks = (T.n + L - 1) / L, per = (nchunks + 63) / 64;
  const long long a = std::min(nchunks, lane * per), b = std::min(nchunks, (lane + 1) * per);
  const unsigned* mp = maps + T.chunk0 * 8;
  int off[ENTRIES], w[ENTRIES];
#pragma unroll
  for (int e = 0; e < ENTRIES; ++e) off[e] = e, w[e] = 0;
  for (long long k = a; k < b; ++k) {  // this lane's run, for every entry offset: the loads do not depend on the state
    const uint4 lo = *reinterpret_cast<const uint4*>(mp + k * 8), hi = *reinterpret_cast<const uint4*>(mp + k * 8 + 4);
#pragma unroll
    for (int e = 0; e < ENTRIES; ++e) {
      const int o = off[e];
      const unsigned v = o == 0 ? lo.x : o == 1 ? lo.y : o == 2 ? lo.z : o == 3 ? lo.w : o == 4 ? hi.x : o == 5 ? hi.y : hi.z;
      off[e] = v & 7;
      w[e] += (int)(v >> 3);
    }
  }
#pragma unroll
  for (int e = 0; e < ENTRIES; ++e) run_off[lane][e] = off[e], run_words[lane][e] = w[e];
  __syncthreads();
  if (lane == 0) {  // chain the 64 runs: a trace starts a word at its first sample
    int o = 0;
    long long base = 0;
    for (int l = 0; l < 64; ++l) {
      run_entry[l] = o;
      run_base[l] = (int)base;
      base += run_words[l][o];
      o = run_off[l][o];
    }
    words[blockIdx.x] = base;
  }
  __syncthreads();
  int o = run_entry[lane], base = run_base[lane];
  for (long long k = a; k < b; ++k) {
    cstate[T.chunk0 + k] = make_int2(o, base);
    const unsigned v = mp[k * 8 + o];
    base += (int)(v >> 3);
    o = v & 7;
  }
}

// ws[chunk0 * L + w]: the first sample (index in its trace) of word w of the trace
__global__ __launch_bounds__(64) void steim_emit_kernel(const EncTrace* __restrict__ tr, const int nt,
                                                        const uint8_t* __restrict__ cls, const int2* __restrict__ cstate,
                                                        int* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) uint8_t s[L];
  __shared__ unsigned sm[NSUB][8];
  __shared__ int sub_entry[NSUB], sub_base[NSUB];
  const int lane = threadIdx.x;
  const long long c = blockIdx.x;
  load_classes(cls, c, s, lane);
  __syncthreads();
  if (lane < NSUB * ENTRIES) sm[lane / ENTRIES][lane % ENTRIES] = walk_sub(s, lane / ENTRIES, lane % ENTRIES);
  __syncthreads();
  if (lane == 0) {
    const int2 st = cstate[c];
    unsigned off = st.x;
    int base = st.y;
    for (int k = 0; k < NSUB; ++k) {
      sub_entry[k] = off;
      sub_base[k] = base;
      const unsigned v = sm[k][off];
      base += (int)(v >> 3);
      off = v & 7;
    }
  }
  __syncthreads();
  if (lane < NSUB) {
    const EncTrace T = tr[owner<false>(tr, nt, c)];
    int* dst = ws + T.chunk0 * L + sub_base[lane];
    const int sample0 = (int)((c - T.chunk0) * L);
    int pos = lane * SUB + sub_entry[lane];
    const int end = (lane + 1) * SUB;
    while (pos < end) {
      const int k = s[pos];
      if (k == 0) break;
      *dst++ = sample0 + pos;  // (a trace has at least as many samples as words: the store stays inside its stretch of ws)
      pos += k;
    }
  }
}

// Every 32-bit word of the data sections: thread g is word g % PW of record g / PW (PW = (reclen - 64) / 4).
__global__ __launch_bounds__(256) void steim_pack_kernel(const int* __restrict__ x, const EncTrace* __restrict__ tr,
                                                         const int nt, const long long* __restrict__ words,
                                                         const uint8_t* __restrict__ cls, const int* __restrict__ ws,
                                                         const int version, const int reclen, const int be,
                                                         const long long total, uint8_t* __restrict__ out,
                                                         int2* __restrict__ rectab) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;  // (total is a multiple of 16: the 16 lanes of a frame leave together)
  const int PW = (reclen - MSEED_DATA_OFFSET) >> 2;
  const long long R = g / PW;
  const int q = (int)(g - R * PW), frame = q >> 4, slot = q & 15;
  const int t = owner<true>(tr, nt, R);
  const EncTrace T = tr[t];
  const long long NW = words[t], W = 15LL * (PW >> 4) - 2;
  const long long w0 = (R - T.rec0) * W;  // the record's first data word: below NW, the trace has ceil(NW / W) records
  const long long P = T.chunk0 * L;
  const int* xs = x + T.first;
  const int k = slot == 0 ? -1 : frame == 0 ? slot - 3 : 13 + (frame - 1) * 15 + slot - 1;
  unsigned word = 0, nib = 0;
  if (k >= 0 && w0 + k < NW) {
    const long long s = ws[P + w0 + k];
    const int c = cls[P + s];
    int bits;
    unsigned dnib = 0;
    if (version == 2) {
      bits = c == 7 ? 4 : c == 6 ? 5 : c == 5 ? 6 : c == 4 ? 8 : c == 3 ? 10 : c == 2 ? 15 : 30;
      nib = c >= 5 ? 3 : c == 4 ? 1 : 2;
      dnib = c == 7 ? 2 : c == 6 ? 1 : c == 5 ? 0 : c == 4 ? 0 : c == 3 ? 3 : c == 2 ? 2 : 1;
    } else {
      bits = c == 4 ? 8 : c == 2 ? 16 : 32;
      nib = c == 4 ? 1 : c == 2 ? 2 : 3;
    }
    int prev = s > 0 ? xs[s - 1] : 0;
    unsigned val = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      if (j < c) {
        const int cur = xs[s + j];
        int d = (int)((unsigned)cur - (unsigned)prev);
        prev = cur;
        if (version == 2 && s == 0 && j == 0 && bits_of(d) > 30) d = 0;
        val = bits == 32 ? (unsigned)d : (val << bits) | ((unsigned)d & ((1u << bits) - 1u));
      }
    }
    word = val | (dnib << 30);
  } else if (frame == 0 && (slot == 1 || slot == 2)) {
    const long long first = ws[P + w0];
    const long long next = w0 + W < NW ? ws[P + w0 + W] : T.n;
    word = (unsigned)(slot == 1 ? xs[first] : xs[next - 1]);  // X0, Xn
    if (slot == 1) rectab[R] = make_int2((int)first, (int)(next - first));
  }
  unsigned ctrl = nib << (30 - 2 * slot);
  ctrl |= __shfl_xor(ctrl, 8, 16);
  ctrl |= __shfl_xor(ctrl, 4, 16);
  ctrl |= __shfl_xor(ctrl, 2, 16);
  ctrl |= __shfl_xor(ctrl, 1, 16);
  if (slot == 0) word = ctrl;
  if (be) word = __builtin_bswap32(word);
  *reinterpret_cast<unsigned*>(out + R * reclen + MSEED_DATA_OFFSET + 4LL * q) = word;
}

// The plain encodings: a fixed count of samples per record, converted and byte-swapped; zeros behind the trace's end.
// ENC 1: int32 -> int16 (two per thread), 3: int32, 4: float32 bits, 5: float64 bits (half a sample per thread).
template <int ENC>
__global__ __launch_bounds__(256) void plain_pack_kernel(const void* __restrict__ x, const EncTrace* __restrict__ tr,
                                                         const int nt, const int reclen, const int be, const long long total,
                                                         uint8_t* __restrict__ out, unsigned long long* __restrict__ bad) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int PW = (reclen - MSEED_DATA_OFFSET) >> 2;
  const long long R = g / PW;
  const int q = (int)(g - R * PW);
  const int t = owner<true>(tr, nt, R);
  const EncTrace T = tr[t];
  const long long r = R - T.rec0;
  unsigned word = 0;
  if (ENC == 3 || ENC == 4) {
    const long long i = r * PW + q;
    if (i < T.n) word = reinterpret_cast<const unsigned*>(x)[T.first + i];
    if (be) word = __builtin_bswap32(word);
  } else if (ENC == 1) {
    const int* xs = reinterpret_cast<const int*>(x) + T.first;
    unsigned h[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long long i = (r * PW + q) * 2 + j;
      if (i < T.n) {
        const int v = xs[i];
        if (v < -32768 || v > 32767) atomicMin(bad, ((unsigned long long)t << 40) | (unsigned long long)i);
        h[j] = (unsigned)v & 0xffffu;
        if (be) h[j] = __builtin_bswap16((unsigned short)h[j]);
      }
    }
    word = h[0] | (h[1] << 16);
  } else {
    const long long i = (r * PW + q) >> 1;
    if (i < T.n) {
      const unsigned long long u = reinterpret_cast<const unsigned long long*>(x)[T.first + i];
      const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
      word = be ? __builtin_bswap32((q & 1) ? lo : hi) : ((q & 1) ? hi : lo);
    }
  }
  *reinterpret_cast<unsigned*>(out + R * reclen + MSEED_DATA_OFFSET + 4LL * q) = word;
}

// ------------------------------------------------------------------------------------------ host
enum { SLOT_SAMPLES, SLOT_CLASSES, SLOT_WORD_STARTS, SLOT_MAPS, SLOT_CHUNK_STATE, SLOT_TABLE, SLOT_FILE, SLOT_RECORDS, ENCODE_SLOTS };
typedef DeviceScratch<ENCODE_SLOTS> EncodeScratch;
EncodeScratch& encode_scratch(int device) {
  static EncodeScratch pool[64];
  return pool[(unsigned)device % 64];
}

// One encode: the traces with samples, what the device holds for them, and the launches.
struct Job {
  const char* who;
  int reclen, enc, be;
  std::vector<EncTrace> tr;       // traces with samples
  std::vector<int64_t> origin;    // their indices in the caller's array
  std::vector<int32_t> factor, mult;
  std::vector<long long> nrec;    // records per trace
  long long chunks = 0, records = 0;
  const void* x = nullptr;
  EncTrace* d_tr = nullptr;
  long long* d_words = nullptr;
  unsigned long long* d_bad = nullptr;
  uint8_t *d_cls = nullptr, *d_out = nullptr;
  int* d_ws = nullptr;
  unsigned* d_maps = nullptr;
  int2 *d_cstate = nullptr, *d_rectab = nullptr;

  bool steim() const { return mseed_is_steim(enc); }
  int nt() const { return (int)tr.size(); }
  size_t table_bytes() const { return tr.size() * (sizeof(EncTrace) + sizeof(long long)) + sizeof(unsigned long long); }
  long long payload_words() const { return records * ((reclen - MSEED_DATA_OFFSET) / 4); }

  int collect(const vp_mseed_trace* traces, int64_t n_traces) {
    for (int64_t t = 0; t < n_traces; ++t) {
      if (traces[t].nsamples <= 0) continue;
      VP_REQUIRE(traces[t].nsamples < (1LL << 31), "%s: trace %lld has %lld samples, the packer indexes 2^31 - 1", who,
                 (long long)t, (long long)traces[t].nsamples);
      int32_t f = 0, m = 0;
      if (const int rc = check_mseed_trace(who, traces[t], t, &f, &m)) return rc;
      tr.push_back(EncTrace{traces[t].first_sample, traces[t].nsamples, chunks, 0});
      chunks += (traces[t].nsamples + L - 1) / L;
      origin.push_back(t);
      factor.push_back(f);
      mult.push_back(m);
    }
    VP_REQUIRE(tr.size() < (1u << 23), "%s: %zu traces in one call", who, tr.size());
    return VP_OK;
  }
  int grow(EncodeScratch& sc, int slot, size_t bytes, void* out) {
    return sc.b[slot].grow(who, bytes ? bytes : 4, bytes / 4 + 4096, (void**)out);
  }
  // the scratch of the stages before the record count is known, and the trace table on the device
  int prepare(EncodeScratch& sc, hipStream_t s) {
    uint8_t* table = nullptr;
    if (const int rc = grow(sc, SLOT_TABLE, table_bytes(), &table)) return rc;
    d_tr = (EncTrace*)table;
    d_words = (long long*)(table + tr.size() * sizeof(EncTrace));
    d_bad = (unsigned long long*)(d_words + tr.size());
    if (steim()) {
      if (const int rc = grow(sc, SLOT_CLASSES, (size_t)chunks * L, &d_cls)) return rc;
      if (const int rc = grow(sc, SLOT_WORD_STARTS, (size_t)chunks * L * sizeof(int), &d_ws)) return rc;
      if (const int rc = grow(sc, SLOT_MAPS, (size_t)chunks * 8 * sizeof(unsigned), &d_maps)) return rc;
      if (const int rc = grow(sc, SLOT_CHUNK_STATE, (size_t)chunks * sizeof(int2), &d_cstate)) return rc;
    }
    VP_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), s));
    return upload_traces(s);
  }
  int upload_traces(hipStream_t s) {
    VP_HIP(hipMemcpyAsync(d_tr, tr.data(), tr.size() * sizeof(EncTrace), hipMemcpyHostToDevice, s));
    return VP_OK;
  }
  // records per trace from the words per trace (Steim) or the samples per record (plain); rec0 of every trace
  void count_records(const std::vector<long long>& words) {
    const long long per = steim() ? mseed_steim_words(reclen) : (reclen - MSEED_DATA_OFFSET) / mseed_plain_width(enc);
    records = 0;
    nrec.resize(tr.size());
    for (size_t t = 0; t < tr.size(); ++t) {
      tr[t].rec0 = records;
      nrec[t] = ((steim() ? words[t] : tr[t].n) + per - 1) / per;
      records += nrec[t];
    }
  }
  int prepare_output(EncodeScratch& sc) {
    if (const int rc = grow(sc, SLOT_FILE, (size_t)records * reclen, &d_out)) return rc;
    if (steim())
      if (const int rc = grow(sc, SLOT_RECORDS, (size_t)records * sizeof(int2), &d_rectab)) return rc;
    return VP_OK;
  }

  void classify(hipStream_t s) const {
    const dim3 grid((unsigned)(chunks * (L / CLASSIFY_BLOCK))), block(CLASSIFY_BLOCK);
    if (enc == 11) hipLaunchKernelGGL(steim_classify_kernel<2>, grid, block, 0, s, (const int*)x, d_tr, nt(), d_cls, d_bad);
    else hipLaunchKernelGGL(steim_classify_kernel<1>, grid, block, 0, s, (const int*)x, d_tr, nt(), d_cls, d_bad);
  }
  void maps(hipStream_t s) const {
    hipLaunchKernelGGL(steim_maps_kernel, dim3((unsigned)chunks), dim3(64), 0, s, d_cls, d_maps);
  }
  void compose(hipStream_t s) const {
    hipLaunchKernelGGL(steim_compose_kernel, dim3((unsigned)nt()), dim3(64), 0, s, d_tr, d_maps, d_cstate, d_words);
  }
  void emit(hipStream_t s) const {
    hipLaunchKernelGGL(steim_emit_kernel, dim3((unsigned)chunks), dim3(64), 0, s, d_tr, nt(), d_cls, d_cstate, d_ws);
  }
  void pack(hipStream_t s) const {
    const long long total = payload_words();
    hipLaunchKernelGGL(steim_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const int*)x, d_tr, nt(),
                       d_words, d_cls, d_ws, enc == 11 ? 2 : 1, reclen, be, total, d_out, d_rectab);
  }
  void plain(hipStream_t s) const {
    const long long total = payload_words();
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (enc == 1) hipLaunchKernelGGL(plain_pack_kernel<1>, grid, block, 0, s, x, d_tr, nt(), reclen, be, total, d_out, d_bad);
    else if (enc == 5) hipLaunchKernelGGL(plain_pack_kernel<5>, grid, block, 0, s, x, d_tr, nt(), reclen, be, total, d_out, d_bad);
    else hipLaunchKernelGGL(plain_pack_kernel<3>, grid, block, 0, s, x, d_tr, nt(), reclen, be, total, d_out, d_bad);
  }
  // Steim: classify, maps, compose, then the words per trace and the out-of-range minimum on the host (one small copy
  // and the call's first wait).  Plain: nothing to run yet.
  int first_half(hipStream_t s, std::vector<long long>* words, unsigned long long* bad) {
    words->assign(tr.size(), 0);
    *bad = ~0ull;
    if (!steim()) return VP_OK;
    VP_REQUIRE(chunks * (L / CLASSIFY_BLOCK) < (1LL << 31), "%s: %lld samples in one call", who, (long long)(chunks * L));
    classify(s);
    maps(s);
    compose(s);
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(words->data(), d_words, tr.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    VP_HIP(hipMemcpyAsync(bad, d_bad, sizeof *bad, hipMemcpyDeviceToHost, s));
    VP_HIP(hipStreamSynchronize(s));
    return VP_OK;
  }
  int second_half(hipStream_t s) {
    VP_REQUIRE((payload_words() + 255) / 256 < (1LL << 31), "%s: %lld records in one call", who, (long long)records);
    if (const int rc = upload_traces(s)) return rc;  // (with rec0)
    if (steim()) {
      emit(s);
      pack(s);
    } else {
      plain(s);
    }
    VP_HIP(hipGetLastError());
    return VP_OK;
  }
};

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_mseed_encode_release_scratch(int device_id, size_t* bytes_freed) {
  return release_scratch("vp_mseed_encode_release_scratch", encode_scratch(device_id), device_id, bytes_freed);
}

extern "C" int vp_mseed_rate_fields(double rate, int32_t* factor, int32_t* multiplier) {
  VP_REQUIRE(factor && multiplier, "vp_mseed_rate_fields: null argument");
  VP_REQUIRE(mseed_rate_fields(rate, factor, multiplier),
             "vp_mseed_rate_fields: sampling rate %.17g has no exact SEED factor / multiplier pair", rate);
  return VP_OK;
}

extern "C" int vp_mseed_record_headers(const vp_mseed_trace* trace, const int64_t* rec_first, const int64_t* rec_count,
                                       int64_t n_records, int64_t first_sequence, int reclen, int encoding, int big_endian,
                                       int b1001_mode, uint8_t* headers) {
  const char* who = "vp_mseed_record_headers";
  VP_REQUIRE(trace && n_records >= 0 && first_sequence >= 0 && (n_records == 0 || (rec_first && rec_count && headers)),
             "%s: null argument", who);
  const int kind = encoding == 4 ? VP_SAMPLES_FLOAT32 : encoding == 5 ? VP_SAMPLES_FLOAT64 : VP_SAMPLES_INT32;
  if (const int rc = check_mseed_encode(who, kind, reclen, encoding, b1001_mode)) return rc;
  int32_t factor = 0, mult = 0;
  if (const int rc = check_mseed_trace(who, *trace, 0, &factor, &mult)) return rc;
  return mseed_trace_headers(who, *trace, rec_first, rec_count, n_records, first_sequence, factor, mult, reclen, encoding,
                             big_endian != 0, b1001_mode, headers, MSEED_DATA_OFFSET);
}

extern "C" int vp_mseed_encode(int device_id, const void* samples, int samples_mem, int sample_kind,
                               const vp_mseed_trace* traces, int64_t n_traces, int reclen, int encoding, int big_endian,
                               int b1001_mode, uint8_t* out_host, size_t out_cap, size_t* out_bytes, int64_t* n_records,
                               int64_t* bad_trace, int64_t* bad_sample) {
  const char* who = "vp_mseed_encode";
  VP_REQUIRE(out_bytes && n_records && bad_trace && bad_sample && n_traces >= 0 && (n_traces == 0 || traces) &&
                 (out_host || out_cap == 0),
             "%s: null argument", who);
  *out_bytes = 0;
  *n_records = 0;
  *bad_trace = *bad_sample = -1;
  VP_REQUIRE(device_id >= 0, "%s: device index", who);
  VP_REQUIRE(samples_mem == VP_MEM_HOST || samples_mem == VP_MEM_DEVICE, "%s: samples_mem %d", who, samples_mem);
  if (const int rc = check_mseed_encode(who, sample_kind, reclen, encoding, b1001_mode)) return rc;
  Job job;
  job.who = who;
  job.reclen = reclen, job.enc = encoding, job.be = big_endian != 0;
  if (const int rc = job.collect(traces, n_traces)) return rc;
  if (job.tr.empty()) return VP_OK;
  VP_REQUIRE(samples, "%s: null samples", who);
  const size_t elem = sample_kind == VP_SAMPLES_FLOAT64 ? 8 : 4;
  VP_REQUIRE(((uintptr_t)samples & (elem - 1)) == 0, "%s: samples are not aligned to their size", who);
  VP_HIP(hipSetDevice(device_id));
  hipStream_t s = nullptr;  // the null stream keeps this call self-contained, as vp_mseed_decode
  EncodeScratch& sc = encode_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  job.x = samples;
  if (samples_mem == VP_MEM_HOST) {
    long long span = 0;
    for (const EncTrace& t : job.tr) {
      VP_REQUIRE(t.first >= 0, "%s: a host trace begins before its array", who);
      span = std::max(span, t.first + t.n);
    }
    void* dx = nullptr;
    if (const int rc = job.grow(sc, SLOT_SAMPLES, (size_t)span * elem, &dx)) return rc;
    VP_HIP(hipMemcpyAsync(dx, samples, (size_t)span * elem, hipMemcpyHostToDevice, s));
    job.x = dx;
  }
  if (const int rc = job.prepare(sc, s)) return rc;
  std::vector<long long> words;
  unsigned long long bad = ~0ull;
  if (const int rc = job.first_half(s, &words, &bad)) return rc;
  const auto refuse = [&](const char* what) {
    const int64_t t = job.origin[(size_t)(bad >> 40)], i = (int64_t)(bad & ((1ull << 40) - 1));
    *bad_trace = t;
    *bad_sample = i;
    set_error("%s: trace %lld, sample %lld: %s", who, (long long)t, (long long)i, what);
    return VP_ERR_INVALID;
  };
  if (bad != ~0ull) return refuse("the difference to the sample before does not fit Steim-2's 30 bits");
  job.count_records(words);
  *n_records = job.records;
  *out_bytes = (size_t)job.records * reclen;
  if (*out_bytes > out_cap) return VP_OK;  // nothing written: the caller comes back with room
  if (const int rc = job.prepare_output(sc)) return rc;
  if (const int rc = job.second_half(s)) return rc;
  std::vector<int2> rectab;
  if (job.steim()) {
    rectab.resize((size_t)job.records);
    VP_HIP(hipMemcpyAsync(rectab.data(), job.d_rectab, rectab.size() * sizeof(int2), hipMemcpyDeviceToHost, s));
  } else if (encoding == 1) {
    VP_HIP(hipMemcpyAsync(&bad, job.d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    VP_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull) return refuse("the sample does not fit int16");
  }
  VP_HIP(hipMemcpyAsync(out_host, job.d_out, *out_bytes, hipMemcpyDeviceToHost, s));
  VP_HIP(hipStreamSynchronize(s));
  // the headers, over the first 64 bytes of every record
  const long long per = job.steim() ? 0 : (reclen - MSEED_DATA_OFFSET) / mseed_plain_width(encoding);
  std::vector<int64_t> first, count;
  for (size_t t = 0; t < job.tr.size(); ++t) {
    const long long r0 = job.tr[t].rec0, nr = job.nrec[t];
    first.resize((size_t)nr);
    count.resize((size_t)nr);
    for (long long r = 0; r < nr; ++r) {
      first[(size_t)r] = job.steim() ? rectab[(size_t)(r0 + r)].x : r * per;
      count[(size_t)r] = job.steim() ? rectab[(size_t)(r0 + r)].y : std::min(per, job.tr[t].n - r * per);
    }
    if (const int rc = mseed_trace_headers(who, traces[job.origin[t]], first.data(), count.data(), nr, 1 + r0, job.factor[t],
                                           job.mult[t], reclen, encoding, job.be != 0, b1001_mode, out_host + r0 * reclen,
                                           reclen))
      return rc;
  }
  return VP_OK;
}

extern "C" int vp_mseed_encode_bench(int device_id, const void* samples_dev, int sample_kind, const vp_mseed_trace* traces,
                                     int64_t n_traces, int reclen, int encoding, int big_endian, int iters, float* ms) {
  const char* who = "vp_mseed_encode_bench";
  VP_REQUIRE(samples_dev && traces && n_traces > 0 && ms && iters > 0 && device_id >= 0, "%s: bad argument", who);
  if (const int rc = check_mseed_encode(who, sample_kind, reclen, encoding, 0)) return rc;
  Job job;
  job.who = who;
  job.reclen = reclen, job.enc = encoding, job.be = big_endian != 0;
  if (const int rc = job.collect(traces, n_traces)) return rc;
  VP_REQUIRE(!job.tr.empty(), "%s: nothing to encode", who);
  VP_HIP(hipSetDevice(device_id));
  BenchTimer t;
  VP_HIP(t.init());
  EncodeScratch& sc = encode_scratch(device_id);
  std::lock_guard<std::mutex> lock(sc.mu);
  job.x = samples_dev;
  if (const int rc = job.prepare(sc, t.s)) return rc;
  std::vector<long long> words;
  unsigned long long bad = ~0ull;
  if (const int rc = job.first_half(t.s, &words, &bad)) return rc;
  VP_REQUIRE(bad == ~0ull, "%s: a sample is out of the encoding's range", who);
  job.count_records(words);
  if (const int rc = job.prepare_output(sc)) return rc;
  if (const int rc = job.second_half(t.s)) return rc;
  for (int k = 0; k < VP_MSEED_ENCODE_STAGES; ++k) ms[k] = 0.f;
  typedef void (Job::*Stage)(hipStream_t) const;
  const Stage stages[VP_MSEED_ENCODE_STAGES] = {&Job::classify, &Job::maps, &Job::compose, &Job::emit, &Job::pack, &Job::plain};
  for (int k = 0; k < VP_MSEED_ENCODE_STAGES; ++k) {
    if ((k < 5) != job.steim()) continue;
    const auto run = [&] {
      (job.*stages[k])(t.s);
      return hipGetLastError();
    };
    VP_HIP(t.run(3, run));
    VP_HIP(t.time(iters, run, &ms[k]));
  }
  VP_HIP(hipStreamSynchronize(t.s));
  return VP_OK;
}
