// Library-wide runtime helpers: ABI version, per-thread last error, device info.
#include "common.hpp"
#include <string.h>
#include <stdlib.h>
#include "kernels.hpp"

namespace vllm {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- runtime options: THE table.  One row per OptionId (kernels.hpp), in the enum's order; a new option is a row here, an id and an
// inline getter there, and its description in include/vllm_hip.h.
OptionValues g_options;
namespace {
struct Option {
    const char *name, *env;   // vllm_set_option's name; the environment variable that gives the first value
    int def;
    enum Rule {
        BOOL,        // stores v != 0
        BOOL_ENV0,   // BOOL, but the environment switches it off by a text that begins with '0' and on by any other (no atoi)
        RANGE,       // stores v where takes(v), the default for any other value on both routes
        REJECT,      // stores v where takes(v); for any other value a set fails with `refusal` and changes nothing, the environment gives the default
        MASK16,      // stores v & 0xffff
    } rule;
    bool (*takes)(int);    // RANGE, REJECT
    const char *refusal;   // REJECT: the error text, printed with the value
};
const Option kOptions[OPT_COUNT] = {
    {"msda_tiled", "VLLM_MSDA_TILED", 1, Option::REJECT, [](int v) { return v == 0 || v == 1 || v == 21; }, "msda_tiled must be one of 0, 1, 21 (got %d)"},
    {"dcnv3_tiled", "VLLM_DCNV3_TILED", 1, Option::RANGE, [](int v) { return v >= 0 && v <= 4; }, nullptr},
    {"dcnv3_bwd_tiled", "VLLM_DCNV3_BWD_TILED", 1, Option::BOOL, nullptr, nullptr},
    {"gemm_half_tail", "VLLM_GEMM_HALF_TAIL", 1, Option::BOOL, nullptr, nullptr},
    {"gemm_res_ring", "VLLM_GEMM_RES_RING", 1, Option::BOOL, nullptr, nullptr},
    {"msda_layer_value_bf16", "VLLM_MSDA_LAYER_VALUE_BF16", 1, Option::BOOL_ENV0, nullptr, nullptr},
    {"gemm_skinny", "VLLM_GEMM_SKINNY", 1, Option::BOOL, nullptr, nullptr},
    {"deform_enc_ffn_slab_rows", "VLLM_DEFORM_ENC_FFN_SLAB_ROWS", 0, Option::REJECT, [](int v) { return v >= 0; }, "deform_enc_ffn_slab_rows must be >= 0 (got %d)"},
    {"msda_layer_fused", "VLLM_MSDA_LAYER_FUSED", 1, Option::BOOL, nullptr, nullptr},
    {"gemm_direct_store", "VLLM_GEMM_DIRECT_STORE", 2, Option::RANGE, [](int v) { return v >= 0 && v <= 2; }, nullptr},
    {"attn_variant", "VLLM_ATTN_VARIANT", 32, Option::MASK16, nullptr, nullptr},
    {"gemm_tile_rb", "VLLM_GEMM_TILE_RB", -1, Option::RANGE, [](int v) { return v >= -1 && v <= 32; }, nullptr},
    {"gemm_variant", "VLLM_GEMM_VARIANT", 0, Option::REJECT, [](int v) { return v >= 0 && v <= 4 && v != 3; }, "gemm_variant must be 0, 1, 2 or 4"},
};
// *out = what `o` stores for `v`; false = it does not take v
bool option_value(const Option &o, int v, int *out)
{
    *out = o.rule == Option::MASK16 ? v & 0xffff : o.takes ? v : v != 0;
    return !o.takes || o.takes(v);
}
}  // namespace
// the first get of an option: its value from the environment (read now, not at load), else the default
int option_from_env(int id)
{
    const Option &o = kOptions[id];
    const char *e = getenv(o.env);
    int v = o.def;
    if (e && o.rule == Option::BOOL_ENV0) v = e[0] != '0';
    else if (e && !option_value(o, atoi(e), &v)) v = o.def;
    return g_options.v[id] = v;
}
}  // namespace vllm

// -> the previous effective value (which reads the environment if nothing has yet), or VLLM_EINVAL
extern "C" int vllm_set_option(const char *name, int value)
{
    if (!name) return VLLM_EINVAL;
    for (int id = 0; id < vllm::OPT_COUNT; ++id) {
        const vllm::Option &o = vllm::kOptions[id];
        if (strcmp(name, o.name)) continue;
        const int old = vllm::option(id);
        int v;
        if (!vllm::option_value(o, value, &v)) {
            if (o.rule == vllm::Option::REJECT) { vllm::set_error(o.refusal, value); return VLLM_EINVAL; }
            v = o.def;
        }
        vllm::g_options.v[id] = v;
        return old;
    }
    vllm::set_error("unknown option %s", name);
    return VLLM_EINVAL;
}
namespace vllm { int dcnv3_pipe_debug_counters(long *out, int n); int gemm256_debug_counters(long *out, int n); int dcnv3_debug_counters(long *out, int n); int msda9_debug_counters(long *out, int n); }
extern "C" int vllm_debug_counters(long *out, int n)
{
    if (!out || n <= 0) { vllm::set_error("vllm_debug_counters: bad arguments"); return VLLM_EINVAL; }
    { static const int gp = [] { const char *e = getenv("VLLM_GEMM_PROF"); return e ? atoi(e) : 0; }(); if (gp) return vllm::gemm256_debug_counters(out, n); }
    if (vllm::dcnv3_tiled_enabled() == 2) return vllm::dcnv3_pipe_debug_counters(out, n);
    if (vllm::dcnv3_tiled_enabled() == 4) return vllm::dcnv3_debug_counters(out, n);
    return vllm::msda9_debug_counters(out, n);
}
// ---- in-step kernel timing ----------------------------------------------------------------------------------------
#include <vector>
#include <mutex>
namespace vllm {
int g_prof_on = 0;
namespace {
std::mutex g_prof_mu;
std::vector<hipEvent_t> g_prof_pool;            // events, reused across read-outs
std::vector<int> g_prof_tags;                   // tag of mark i (event i)
}
void prof_mark_slow(int tag, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    const size_t i = g_prof_tags.size();
    if (i >= (1u << 20)) return;                // bounded: a forgotten vllm_prof_enable(1) must not eat the host's memory
    if (i >= g_prof_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        g_prof_pool.push_back(e);
    }
    if (hipEventRecord(g_prof_pool[i], st) == hipSuccess) g_prof_tags.push_back(tag);
}
}  // namespace vllm
static const char *const kProfNames[vllm::PT_COUNT] = {"end", "embed", "norm", "gemm_qkv", "qk_norm", "attn", "gemm_proj", "gemm_fc1",
                                                        "gemm_fc2", "gemm_bridge", "bridge_other", "msda_encoder_shape", "msda_other",
                                                        "msda_layer"};
extern "C" int vllm_prof_enable(int on)
{
    std::lock_guard<std::mutex> lk(vllm::g_prof_mu);
    vllm::g_prof_tags.clear();
    vllm::g_prof_on = on != 0;
    return vllm::PT_COUNT;
}
extern "C" const char *vllm_prof_tag_name(int tag) { return tag >= 0 && tag < vllm::PT_COUNT ? kProfNames[tag] : ""; }
extern "C" int vllm_prof_read(double *us_sum, long *count, int n)
{
    if (!us_sum || !count || n < vllm::PT_COUNT) { vllm::set_error("vllm_prof_read: need %d slots", (int)vllm::PT_COUNT); return VLLM_EINVAL; }
    std::lock_guard<std::mutex> lk(vllm::g_prof_mu);
    for (int i = 0; i < n; ++i) { us_sum[i] = 0.0; count[i] = 0; }
    const size_t m = vllm::g_prof_tags.size();
    if (m && hipEventSynchronize(vllm::g_prof_pool[m - 1]) != hipSuccess) { vllm::set_error("vllm_prof_read: event wait failed"); return VLLM_ELAUNCH; }
    for (size_t i = 0; i + 1 < m; ++i) {
        const int tag = vllm::g_prof_tags[i];
        if (tag == vllm::PT_END) continue;      // the gap between two C calls belongs to the host, not to a kernel
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, vllm::g_prof_pool[i], vllm::g_prof_pool[i + 1]) != hipSuccess) continue;
        us_sum[tag] += (double)ms * 1e3;
        count[tag] += 1;
    }
    vllm::g_prof_tags.clear();
    return vllm::PT_COUNT;
}
extern "C" int vllm_abi_version(void) { return VLLM_ABI_VERSION; }
extern "C" const char *vllm_last_error(void) { return vllm::g_err; }
extern "C" int vllm_device_info(char *name, int cap)
{
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        vllm::set_error("no HIP device");
        return VLLM_ELAUNCH;
    }
    if (name && cap > 0) {
        strncpy(name, prop.gcnArchName, cap - 1);
        name[cap - 1] = 0;
    }
    return prop.multiProcessorCount;
}
