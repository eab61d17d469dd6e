// Stand-alone check of vp_mseed_scan (volpick_amd/csrc/mseed.hip) under host threads, meant for ThreadSanitizer: eight
// std::threads scan one shared miniSEED buffer, no scan before they start, so that the first concurrent calls are the ones
// that build the scanner's static CRC-32C tables.  tests/test_mseed_scan_tsan_cpu.py writes the file (miniSEED 2 and
// miniSEED 3 records mixed), builds this together with mseed.hip under -fsanitize=thread and runs it:
//     mseed_scan_threads FILE
// Calls vp_mseed_scan and vp::set_error only: no HIP function, no GPU.  Prints "N threads, M records, identical" and
// returns 0, or a line per difference and 1.  A ThreadSanitizer report goes to stderr.
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "vp_error.h"

// The error text of the library, as volpick_amd/csrc/net.hip keeps it.
namespace vp {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }

}  // namespace vp

constexpr int THREADS = 8, ROUNDS = 20;
constexpr int64_t CAP = 4096;

static std::atomic<int> g_ready{0};
static std::atomic<int> g_bad{0};

static void fail(int thread, int round, const char* what) {
  ++g_bad;
  std::printf("DIFFERENT thread %d round %d: %s\n", thread, round, what);
}

struct Table {
  int rc = 0;
  int64_t n = -1;
  std::vector<vp_mseed_record> recs;
  bool operator==(const Table& o) const {
    return rc == o.rc && n == o.n && std::memcmp(recs.data(), o.recs.data(), (size_t)CAP * sizeof(vp_mseed_record)) == 0;
  }
};

static Table scan(const std::vector<uint8_t>& file) {
  Table t;
  t.recs.resize((size_t)CAP);
  std::memset(t.recs.data(), 0, (size_t)CAP * sizeof(vp_mseed_record));  // padding bytes too
  t.rc = vp_mseed_scan(file.data(), file.size(), t.recs.data(), CAP, &t.n);
  return t;
}

// A refusal whose text names byte `offset`: 64-byte steps of zeros (the scanner walks over them), then a header.
static std::vector<uint8_t> truncated_v3(size_t offset) {  // a miniSEED 3 header whose payload runs past the end
  std::vector<uint8_t> b(offset + 40, 0);
  b[offset] = 'M', b[offset + 1] = 'S', b[offset + 2] = 3;
  b[offset + 36] = 100;
  return b;
}
static std::vector<uint8_t> no_blockette_1000(size_t offset) {  // a miniSEED 2 data header with an empty blockette chain
  std::vector<uint8_t> b(offset + 64, 0);
  std::memcpy(&b[offset], "000001D", 7);
  return b;
}

static void refuse(int thread, int round, const std::vector<uint8_t>& b, const std::string& want) {
  vp_mseed_record rec;
  int64_t n = -7;
  const int rc = vp_mseed_scan(b.data(), b.size(), &rec, 1, &n);
  if (rc != VP_ERR_INVALID) fail(thread, round, "a refusal was accepted");
  std::this_thread::yield();  // the text is the thread's until its next call, whatever the others do meanwhile
  if (want != vp::last_error()) {
    fail(thread, round, "the thread's error text is not its own");
    std::printf("  want '%s'\n  have '%s'\n", want.c_str(), vp::last_error());
  }
}

static void worker(int k, const std::vector<uint8_t>* file, Table* first) {
  const size_t off3 = 64 * (size_t)(1 + k), off2 = 64 * (size_t)(101 + k);  // offsets no other thread uses
  const std::vector<uint8_t> b3 = truncated_v3(off3), b2 = no_blockette_1000(off2);
  const std::string want3 = "miniSEED 3 record at byte " + std::to_string(off3) + " runs past the end of the buffer";
  const std::string want2 = "mseed record at byte " + std::to_string(off2) + " has no (valid) blockette 1000";
  ++g_ready;
  while (g_ready.load() < THREADS) std::this_thread::yield();  // all together into the first scan
  for (int r = 0; r < ROUNDS; ++r) {
    Table t = scan(*file);
    if (r == 0)
      *first = std::move(t);
    else if (!(t == *first))
      fail(k, r, "the record table differs from this thread's first");
    refuse(k, r, b3, want3);
    refuse(k, r, b2, want2);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: mseed_scan_threads FILE\n");
    return 2;
  }
  std::vector<uint8_t> file;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    uint8_t chunk[4096];
    for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + got);
    std::fclose(f);
  }
  if (file.empty()) {
    std::printf("DIFFERENT: nothing read from %s\n", argv[1]);
    return 1;
  }
  std::vector<Table> first(THREADS);
  std::vector<std::thread> threads;
  for (int k = 0; k < THREADS; ++k) threads.emplace_back(worker, k, &file, &first[k]);
  for (std::thread& t : threads) t.join();
  int n_v2 = 0, n_v3 = 0;
  if (first[0].rc != VP_OK || first[0].n < 1 || first[0].n > CAP) {
    fail(0, 0, "the scan of the file failed, found nothing or more than the table holds");
  } else {
    for (int64_t i = 0; i < first[0].n; ++i) (first[0].recs[(size_t)i].quality >= 0x300 ? n_v3 : n_v2)++;
    if (n_v2 == 0 || n_v3 == 0) fail(0, 0, "the file does not hold both miniSEED 2 and miniSEED 3 records");
  }
  for (int k = 1; k < THREADS; ++k)
    if (!(first[k] == first[0])) fail(k, 0, "the record table differs from the first thread's");
  if (g_bad.load()) return 1;
  std::printf("%d threads, %lld records, identical\n", THREADS, (long long)first[0].n);
  return 0;
}
