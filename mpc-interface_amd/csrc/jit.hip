// jit.hip -- the persistent assembly kernel compiled for ONE plan (host side).
//
// The reference re-interprets its problem description on every tick; the plan compiler
// turns the description into tables once; this file goes one step further for plans that
// assemble large batches: it hands the persistent kernel's own source (resident.hip, the very
// file that is also built ahead of time) to hiprtc together with a generated "plan_spec.h"
// that states the plan's sizes, every wavefront's list of matrix-core trips, the fetch tables as
// runs of streams (so that a workgroup asks for its first inputs without reading a table first) and
// the records of the systems whose horizon tables are built on chip as constants.
// What the ahead-of-time kernel interprets per instance -- trip records, flags, loop bounds,
// kernel-argument reloads -- folds away: a trip is eight 8-byte LDS reads at immediate
// offsets and four MFMAs.  The result is cached per plan structure; the ahead-of-time kernel
// remains the fallback (no hiprtc, a compile failure, small batches) and the parity reference
// (tests run both, MPCASM_OPT_JIT).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "jit.h"
#include "kernels.h"

namespace mpcasm {

namespace {

#include "jit_embed.inc"  // k_src_resident, k_src_device_prims, k_src_plan_dev, k_src_plan_tables

// (the per-plan kernel is the faster one at every size -- C2: 11.7 against 20.3 us at B = 512, 30.4
// against 56 at 4 096 -- the threshold only keeps one-off small uses, the B = 1 drop-in calls,
// from paying the 1-4 s of a compilation)
constexpr int JIT_MIN_BATCH = 512;

// ---- hiprtc, loaded on first use (no link-time dependency) ------------------------------
struct Rtc {
  typedef struct _hiprtcProgram* Program;
  int (*create)(Program*, const char*, const char*, int, const char* const*, const char* const*);
  int (*compile)(Program, int, const char* const*);
  int (*log_size)(Program, size_t*);
  int (*get_log)(Program, char*);
  int (*code_size)(Program, size_t*);
  int (*get_code)(Program, char*);
  int (*destroy)(Program*);
  bool ok = false;
};

const Rtc& rtc() {
  static Rtc r;
  static std::once_flag once;
  std::call_once(once, [] {
    void* lib = nullptr;
    for (const char* name : {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) return;
    auto sym = [&](const char* name) { return dlsym(lib, name); };
    r.create = reinterpret_cast<decltype(r.create)>(sym("hiprtcCreateProgram"));
    r.compile = reinterpret_cast<decltype(r.compile)>(sym("hiprtcCompileProgram"));
    r.log_size = reinterpret_cast<decltype(r.log_size)>(sym("hiprtcGetProgramLogSize"));
    r.get_log = reinterpret_cast<decltype(r.get_log)>(sym("hiprtcGetProgramLog"));
    r.code_size = reinterpret_cast<decltype(r.code_size)>(sym("hiprtcGetCodeSize"));
    r.get_code = reinterpret_cast<decltype(r.get_code)>(sym("hiprtcGetCode"));
    r.destroy = reinterpret_cast<decltype(r.destroy)>(sym("hiprtcDestroyProgram"));
    r.ok = r.create && r.compile && r.log_size && r.get_log && r.code_size && r.get_code && r.destroy;
  });
  return r;
}

void append(std::string& s, const char* fmt, long long v) {
  char buf[96];
  snprintf(buf, sizeof buf, fmt, v);
  s += buf;
}

}  // namespace

// One chunk of a fetch table -- `lanes` entries (stream, byte offset), one per lane of an LDS-DMA load --
// as maximal runs: FS_WORDS words each, (first lane, lanes, stream, first byte, bytes per lane step,
// period in lanes).  Lane l of a run reads byte `first byte + ((l - first lane) % period) * step` of its
// stream; a plain run has period = lanes, the padding (the plan's two constants over and over) a period
// of 1, 2 or 4 lanes.  The runs are taken greedily, the longest that starts at each lane.
std::vector<int32_t> jit_fetch_segments(const int32_t* meta, int lanes) {
  std::vector<int32_t> out;
  for (int i = 0; i < lanes;) {
    const int stream = meta[2 * i], byte0 = meta[2 * i + 1];
    const int step = i + 1 < lanes && meta[2 * (i + 1)] == stream ? meta[2 * (i + 1) + 1] - byte0 : 0;
    int best = 0, best_period = 0;
    for (int period : {0, 4, 2, 1}) {  // (0: plain; a tie goes to the earlier form)
      int n = 0;
      while (i + n < lanes && meta[2 * (i + n)] == stream &&
             meta[2 * (i + n) + 1] == byte0 + (period ? n % period : n) * (period == 1 ? 0 : step))
        ++n;
      if (n > best) best = n, best_period = period;
    }
    const int period = best_period && best_period < best ? best_period : best;
    out.insert(out.end(), {i, best, stream, byte0, best > 1 && period > 1 ? step : 0, period});
    i += best;
  }
  return out;
}

// The fetch tables of a plan by chunks, for the per-plan kernel: per chunk of the (A, B) slot (32 doubles
// = 64 lanes of 4 bytes), then per chunk of the image, its runs -- or none when it has more than `limit`
// (at most FS_MAX): that chunk stays on the table.  Returned as [kind (0: (A, B), 1: image), chunk, runs,
// runs x FS_WORDS words] per chunk.
std::vector<int32_t> jit_fetch_plan(const PlanDev& d, const int32_t* it, int limit) {
  std::vector<int32_t> out;
  if (limit > FS_MAX) limit = FS_MAX;
  for (int kind = 0; kind < 2; ++kind) {
    const int chunks = kind == 0 ? d.rs_ab / 32 : d.rs_nchunk;
    const int32_t* meta = it + (kind == 0 ? d.off_rs_abmeta : d.off_rs_inmeta);
    for (int k = 0; k < chunks; ++k) {
      std::vector<int32_t> segs = jit_fetch_segments(meta + k * 128, 64);
      // (the image's table-path chunks are kept as a 32-bit mask in the kernel)
      if ((int)segs.size() > limit * FS_WORDS || (kind == 1 && k >= 32)) segs.clear();
      out.insert(out.end(), {kind, k, (int32_t)(segs.size() / FS_WORDS)});
      out.insert(out.end(), segs.begin(), segs.end());
    }
  }
  return out;
}

// The constants of one plan as a header: PlanConst mirrors PlanDev's int fields (same names,
// so the kernel body reads `p.no` either way), JC picks the compose-slot count the ahead-of-time
// build would, TRIPS / WTRIP are the trip records (plan_tables.h RT_*) and the per-wavefront
// ranges.
std::string jit_spec_header(const PlanDev& d, const int32_t* it, int seg_limit) {
  std::string s = "// generated by libmpcasm (jit.hip) for one plan\n#pragma once\n"
                  "namespace mpcasm {\nnamespace spec {\nstruct PlanConst {\n";
#define MPCASM_X(f, ...) append(s, "  static constexpr int " #f " = %lld;\n", (long long)d.f);
  MPCASM_PLAN_INT_FIELDS(MPCASM_X, MPCASM_X)
#undef MPCASM_X
  append(s, "  static constexpr unsigned rs_src16 = %lldu;\n};\n", (long long)d.rs_src16);
  const int jc = d.rs_jc <= 3 ? 3 : d.rs_jc <= 4 ? 4 : d.rs_jc <= 5 ? 5 : d.rs_jc <= 8 ? 8 : RS_JC_MAX;
  append(s, "constexpr int JC = %lld;\n", jc);
  append(s, "constexpr int NTRIP = %lld;\n", d.rs_ntrip);
  s += "constexpr int TRIPS[NTRIP + 1][8] = {\n";
  const int32_t* tr = it + d.off_rs_trip;
  for (int t = 0; t <= d.rs_ntrip; ++t) {  // (one spare all-zero record)
    s += "  {";
    for (int k = 0; k < RS_TRIP_WORDS; ++k) append(s, k ? ", %lld" : "%lld", tr[t * RS_TRIP_WORDS + k]);
    s += "},\n";
  }
  s += "};\nconstexpr int WTRIP[8][2] = {";
  const int32_t* wt = it + d.off_rs_wtrip;
  for (int w = 0; w < RS_WAVES; ++w) {
    append(s, "{%lld, ", wt[2 * w]);
    append(s, "%lld}, ", wt[2 * w + 1]);
  }
  s += "};\n";
  // the input fetch by arithmetic: the runs of every chunk of the (A, B) slot and of the image
  // (FSEG_*_N[chunk] = 0: that chunk stays on the table), see jit_fetch_segments
  const std::vector<int32_t> fetch = jit_fetch_plan(d, it, seg_limit);
  for (int kind = 0; kind < 2; ++kind) {
    const int chunks = kind == 0 ? d.rs_ab / 32 : d.rs_nchunk;
    const char* name = kind == 0 ? "AB" : "IMG";
    std::string counts, table;
    long long on_table = 0;
    for (size_t at = 0; at < fetch.size(); at += 3 + fetch[at + 2] * FS_WORDS) {
      if (fetch[at] != kind) continue;
      const int n = fetch[at + 2];
      if (n == 0 && fetch[at + 1] < 32) on_table |= 1ll << fetch[at + 1];
      append(counts, "%lld, ", n);
      table += "  {";
      for (int g = 0; g < FS_MAX; ++g) {
        table += "{";
        for (int w = 0; w < FS_WORDS; ++w) append(table, w ? ", %lld" : "%lld", g < n ? fetch[at + 3 + g * FS_WORDS + w] : 0);
        table += "}, ";
      }
      table += "},\n";
    }
    if (chunks == 0) counts = "0", table = "  {},\n";
    s += std::string("constexpr int FSEG_") + name + "_N[] = {" + counts + "};\n";
    s += std::string("constexpr int FSEG_") + name + "[][8][6] = {\n" + table + "};\n";
    // bit k: chunk k is fetched through the table (chunks from 32 on always are)
    s += std::string("constexpr unsigned FSEG_") + name + "_TABLE = ";
    append(s, "%lldu;\n", on_table);
  }
  // the records of the generated systems (plan_tables.h LT_*)
  s += "constexpr int LTI[4][8] = {\n";
  for (int g = 0; g < RS_LTI_MAX; ++g) {
    s += "  {";
    for (int w = 0; w < RS_LTI_WORDS; ++w)
      append(s, w ? ", %lld" : "%lld", g < d.rs_nlti ? it[d.off_rs_lti + g * RS_LTI_WORDS + w] : 0);
    s += "},\n";
  }
  s += "};\n}  // namespace spec\n}  // namespace mpcasm\n";
  return s;
}

// hiprtc: resident.hip + the generated header -> a gfx950 code object
int jit_compile(const std::string& header, std::vector<char>* code, std::string* log, bool stamps,
                int phases) {
  const Rtc& r = rtc();
  if (!r.ok) {
    if (log) *log = "libhiprtc.so could not be loaded";
    return MPCASM_ERR_LIMIT;
  }
  const char* headers[] = {header.c_str(), k_src_device_prims, k_src_plan_dev, k_src_plan_tables};
  const char* names[] = {"plan_spec.h", "device_prims.h", "plan_dev.h", "plan_tables.h"};
  Rtc::Program prog = nullptr;
  if (r.create(&prog, k_src_resident, "resident.hip", 4, headers, names) != 0) return MPCASM_ERR_HIP;
  // (tuning aid: MPCASM_JIT_WAVES_PER_EU=6 asks for a register budget that lets a third
  // workgroup share a CU)
  const char* waves = getenv("MPCASM_JIT_WAVES_PER_EU");
  const std::string wopt = std::string("-DMPCASM_SPEC_WAVES_PER_EU=") + (waves ? waves : "4");
  // (A/B aid: MPCASM_JIT_PLAIN_STORES=1 compiles the kernel with ordinary result stores)
  const char* last = stamps ? "-DMPCASM_SPEC_STAMPS=1"
                            : (getenv("MPCASM_JIT_PLAIN_STORES") ? "-DMPCASM_PLAIN_STORES=1" : "-DMPCASM_SPEC_NT=1");
  char popt[48];
  snprintf(popt, sizeof popt, "-DMPCASM_SPEC_PHASES=%d", phases);
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-DMPCASM_SPEC=1", wopt.c_str(), last, popt};
  const int rc = r.compile(prog, phases >= 0 ? 7 : 6, opts);
  size_t n = 0;
  if (log && r.log_size(prog, &n) == 0 && n > 1) {
    log->resize(n);
    r.get_log(prog, &(*log)[0]);
  }
  int out = MPCASM_ERR_HIP;
  if (rc == 0 && r.code_size(prog, &n) == 0 && n > 0) {
    code->resize(n);
    if (r.get_code(prog, code->data()) == 0) out = MPCASM_OK;
  }
  r.destroy(&prog);
  if (const char* dump = getenv("MPCASM_JIT_DUMP")) {  // diagnostic: <dump>.h, <dump>.co
    const std::string base(dump);
    if (FILE* f = fopen((base + ".h").c_str(), "w")) {
      fwrite(header.data(), 1, header.size(), f);
      fclose(f);
    }
    if (out == MPCASM_OK)
      if (FILE* f = fopen((base + ".co").c_str(), "wb")) {
        fwrite(code->data(), 1, code->size(), f);
        fclose(f);
      }
  }
  return out;
}

namespace {

// ---- code objects on disk ------------------------------------------------------------------
// A compilation takes 1-4 s; its result depends on nothing but the text handed to hiprtc (the
// generated header, the embedded sources, the options) and on the compiler.  So the code object
// is kept under $MPCASM_CACHE_DIR, else $XDG_CACHE_HOME/mpcasm, else ~/.cache/mpcasm, named by
// a hash of all of that: the eight ranks of a node and every later process load it instead of
// compiling again.  MPCASM_NO_DISK_CACHE=1 turns it off.  Files are written under a temporary
// name and renamed, so a reader never sees half a file; a file that does not load is deleted and compiled afresh.
std::atomic<long> g_stat_compiled{0}, g_stat_disk_hits{0}, g_stat_disk_writes{0};

uint64_t fnv1a(const std::string& text, uint64_t h) {
  for (unsigned char c : text) {
    h ^= c;
    h *= 1099511628211ull;
  }
  return h;
}

std::string cache_dir() {
  if (const char* off = getenv("MPCASM_NO_DISK_CACHE"))
    if (off[0] && off[0] != '0') return "";
  std::string dir;
  if (const char* d = getenv("MPCASM_CACHE_DIR")) {
    dir = d;
  } else if (const char* x = getenv("XDG_CACHE_HOME")) {
    dir = std::string(x) + "/mpcasm";
  } else if (const char* home = getenv("HOME")) {
    dir = std::string(home) + "/.cache/mpcasm";
  }
  if (dir.empty()) return "";
  // (mkdir -p of the last two levels is enough for the three forms above)
  const size_t cut = dir.find_last_of('/');
  if (cut != std::string::npos && cut > 0) (void)mkdir(dir.substr(0, cut).c_str(), 0755);
  (void)mkdir(dir.c_str(), 0755);
  struct stat st;
  if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || access(dir.c_str(), W_OK) != 0) return "";
  return dir;
}

std::string cache_key(const std::string& header, const std::string& options) {
  int major = 0, minor = 0;
  if (void* lib = dlopen("libhiprtc.so", RTLD_NOW | RTLD_NOLOAD)) {
    typedef int (*version_fn)(int*, int*);
    if (auto f = reinterpret_cast<version_fn>(dlsym(lib, "hiprtcVersion"))) (void)f(&major, &minor);
  }
  std::string all = header + "\x1f" + options + "\x1f" + k_src_resident + "\x1f" + k_src_device_prims +
                    "\x1f" + k_src_plan_dev + "\x1f" + k_src_plan_tables + "\x1fhiprtc " +
                    std::to_string(major) + "." + std::to_string(minor);
  // (a code object of another patch release may not load: the runtime's own version too)
  int runtime = 0;
  if (hipRuntimeGetVersion(&runtime) == hipSuccess) all += " hip " + std::to_string(runtime);
  char name[64];
  snprintf(name, sizeof name, "%016llx%016llx", (unsigned long long)fnv1a(all, 14695981039346656037ull),
           (unsigned long long)fnv1a(all, 0x9E3779B97F4A7C15ull));
  return name;
}

bool disk_read(const std::string& path, std::vector<char>* code) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  bool ok = n > 0;
  if (ok) {
    code->resize((size_t)n);
    ok = fread(code->data(), 1, (size_t)n, f) == (size_t)n;
  }
  fclose(f);
  return ok;
}

void disk_write(const std::string& path, const std::vector<char>& code) {
  const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) return;
  const bool ok = fwrite(code.data(), 1, code.size(), f) == code.size();
  fclose(f);
  if (ok && rename(tmp.c_str(), path.c_str()) == 0)
    ++g_stat_disk_writes;
  else
    (void)unlink(tmp.c_str());
}

struct JitKernel {
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  int per_cu = 0;
  size_t lds = 0;
  bool failed = false;
  bool building = true;  // (under g_mutex) the thread that created the slot is still compiling
};

std::mutex g_mutex;
std::condition_variable g_built;
// one compiled kernel per (device, plan structure); the key is the generated header itself
std::map<std::pair<int, std::string>, JitKernel*> g_cache;
// ... found again without generating that header (10 KB of text per launch otherwise): by the
// plan's own device tables, which identify it while it lives (jit_forget when it dies), and what
// else selects a build
struct FastKey {
  const void* itab;
  int device, p_direct, phases, fetch_runs;
  bool operator<(const FastKey& o) const {
    if (fetch_runs != o.fetch_runs) return fetch_runs < o.fetch_runs;
    if (itab != o.itab) return itab < o.itab;
    if (device != o.device) return device < o.device;
    if (p_direct != o.p_direct) return p_direct < o.p_direct;
    return phases < o.phases;
  }
};
std::map<FastKey, JitKernel*> g_fast;

}  // namespace

// The code object of one generated header: from the disk cache, else compiled (and stored).
// Called WITHOUT g_mutex: a compilation must not hold up the launches of other plans.
bool jit_code_for(const std::string& header, bool stamps, int phases, std::vector<char>* code,
                  std::string* log_out, bool distrust_disk) {
  const char* waves = getenv("MPCASM_JIT_WAVES_PER_EU");
  const std::string options = std::string(stamps ? "stamps " : "") + "phases " + std::to_string(phases) +
                              " waves " + (waves ? waves : "4") +
                              (getenv("MPCASM_JIT_PLAIN_STORES") ? " plain-stores" : "");
  const std::string dir = cache_dir();
  const std::string path = dir.empty() ? "" : dir + "/" + cache_key(header, options) + ".co";
  if (distrust_disk && !path.empty()) (void)unlink(path.c_str());  // (it was read and did not load)
  if (!distrust_disk && !path.empty() && disk_read(path, code)) {
    ++g_stat_disk_hits;
    if (getenv("MPCASM_JIT_VERBOSE")) fprintf(stderr, "mpcasm: jit: code object from %s\n", path.c_str());
    return true;
  }
  std::string log;
  const int rc = jit_compile(header, code, &log, stamps, phases);
  if (log_out) *log_out = log;
  if (rc != MPCASM_OK) {
    if (getenv("MPCASM_JIT_VERBOSE")) fprintf(stderr, "mpcasm: jit failed:\n%s\n", log.c_str());
    return false;
  }
  ++g_stat_compiled;
  if (getenv("MPCASM_JIT_VERBOSE")) fprintf(stderr, "mpcasm: jit: compiled (%zu bytes)\n", code->size());
  if (!path.empty()) disk_write(path, *code);
  return true;
}

namespace {
}  // namespace

// the specialised kernel of this plan on this device, compiled on first use; nullptr when the
// plan runs on the ahead-of-time kernel (JIT off, batch too small, hiprtc missing, a failure)
const void* jit_kernel_for(const PlanDev& d, const int32_t* h_itab, int device, int batch,
                           size_t lds_bytes, int jit, int phase_mask, int fetch_runs) {
  if (jit == 2) return nullptr;
  const bool stamps = (phase_mask & 64) != 0;  // the diagnostic build with in-kernel cycle stamps
  // (the phase mask is a constant of the build: the shipped value in every normal process, one
  // more build per value a profiling tool sets)
  const int phases = stamps ? -1 : phase_mask;
  const FastKey fast{d.itab, stamps ? device + 4096 : device, d.rs_p_direct, phases, fetch_runs};
  // a small launch does not start a compilation, but takes the kernel when it is there already
  // (mpcasm_plan_prepare, or an earlier large launch)
  const bool may_build = jit == 1 || batch >= JIT_MIN_BATCH;
  JitKernel* slot = nullptr;
  bool mine = false;
  std::string header;
  {
    std::unique_lock<std::mutex> lock(g_mutex);
    auto found = g_fast.find(fast);
    if (found != g_fast.end()) {
      slot = found->second;
    } else if (may_build) {
      // by the generated header's text: another plan of the same structure may have built it
      header = jit_spec_header(d, h_itab, fast.fetch_runs);
      JitKernel*& by_text = g_cache[std::make_pair(fast.device, header + "//" + std::to_string(phases))];
      if (by_text == nullptr) {
        by_text = new JitKernel();
        mine = true;
      }
      slot = by_text;
      g_fast[fast] = slot;
    } else {
      return nullptr;
    }
    if (!mine) {
      if (slot->building && !may_build) return nullptr;  // (do not wait for a compilation either)
      g_built.wait(lock, [&] { return !slot->building; });
    }
  }
  if (mine) {  // compile (or read from disk) and load, outside the lock; then publish
    std::vector<char> code;
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    bool ok = false;
    for (int attempt = 0; attempt < 2 && !ok; ++attempt) {
      // a code object from the disk cache that does not load (another ROCm patch release wrote it)
      // is deleted and compiled afresh, once
      code.clear();
      const long hits = g_stat_disk_hits;
      ok = jit_code_for(header, stamps, phases, &code, nullptr, attempt == 1);
      const bool from_disk = g_stat_disk_hits != hits;
      if (ok && (hipModuleLoadData(&module, code.data()) != hipSuccess ||
                 hipModuleGetFunction(&fn, module, "resident_spec_kernel") != hipSuccess)) {
        (void)hipGetLastError();
        if (module) (void)hipModuleUnload(module);
        module = nullptr;
        fn = nullptr;
        ok = false;
        if (!from_disk) break;
      } else if (!ok) {
        break;
      }
    }
    // the dynamic-LDS limit of the function: raised once, here, to the CU's whole LDS
    if (ok && hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  CU_LDS_BYTES) != hipSuccess) {
      (void)hipGetLastError();  // (this runtime grants 156 KiB, not the CU's whole 160: capi.hip allow_whole_lds)
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                              RESIDENT_LDS_LIMIT) != hipSuccess) {
        (void)hipGetLastError();
        ok = false;
      }
    }
    {
      std::lock_guard<std::mutex> lock(g_mutex);
      slot->module = module;
      slot->fn = fn;
      slot->failed = !ok;
      slot->building = false;
    }
    g_built.notify_all();
  }
  std::lock_guard<std::mutex> lock(g_mutex);
  if (slot->failed) return nullptr;
  if (slot->lds != lds_bytes) {
    int n = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, slot->fn, RS_NT, lds_bytes) != hipSuccess ||
        n < 1) {
      (void)hipGetLastError();
      slot->failed = true;
      return nullptr;
    }
    slot->per_cu = n;
    slot->lds = lds_bytes;
  }
  return slot;
}

bool jit_available() { return rtc().ok; }

void jit_stats(long out[3]) {
  out[0] = g_stat_compiled;
  out[1] = g_stat_disk_hits;
  out[2] = g_stat_disk_writes;
}

// a plan is gone: its device tables no longer identify anything
void jit_forget(const void* itab) {
  std::lock_guard<std::mutex> lock(g_mutex);
  for (auto it = g_fast.begin(); it != g_fast.end();)
    it = it->first.itab == itab ? g_fast.erase(it) : std::next(it);
}

int jit_launch(const void* kernel, const PlanDev& p, const AssembleCall& call) {
  const JitKernel* k = static_cast<const JitKernel*>(kernel);
  AssembleCall c = call;  // (hipModuleLaunchKernel takes the arguments' addresses as void*)
  int per_cu = k->per_cu;
  if (c.opt.per_cu > 0 && c.opt.per_cu < per_cu) per_cu = c.opt.per_cu;
  long grid = (long)c.num_cus * per_cu;
  if (c.opt.grid > 0 && c.opt.grid < grid) grid = c.opt.grid;
  if (grid > c.batch) grid = c.batch;
  const int32_t* itab = p.itab;
  const double* dtab = p.dtab;
  SrcTable s = c.src;
  unsigned long long* stamps = (c.opt.phase_mask & 64) ? static_cast<unsigned long long*>(c.work) : nullptr;
  void* args[] = {&itab, &dtab, &s, &c.params, &c.given, &c.P, &c.q, &c.G, &c.h, &c.batch, &c.opt.phase_mask, &stamps};
  *c.err = hipModuleLaunchKernel(k->fn, (unsigned)grid, 1, 1, RS_NT, 1, 1, (unsigned)k->lds, c.stream,
                                 args, nullptr);
  return *c.err == hipSuccess ? MPCASM_OK : MPCASM_ERR_HIP;
}

}  // namespace mpcasm
