// Kernel launch log (kernel_log.h): hnsw_kernel_log, hnsw_kernel_log_get, hnsw_kernel_name.
#include "kernel_log.h"

#include <cxxabi.h>
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/hnsw_mi355x.h"

namespace hx {

std::atomic<int> g_klog_on{0};

namespace {
std::mutex g_klog_mu;
std::map<const void *, uint64_t> g_klog;  // kernel (host-side pointer) -> launches since recording started

void erase_all(std::string &s, const char *what) {
    const size_t n = strlen(what);
    for (size_t p; (p = s.find(what)) != std::string::npos;) s.erase(p, n);
}

// the device-side name the runtime registered for a kernel pointer (mangled), else the host symbol's
std::string raw_name(const void *kern) {
    if (const char *s = hipKernelNameRefByPtr(kern, nullptr)) return s;
    (void)hipGetLastError();
    Dl_info info{};
    if (dladdr(kern, &info) && info.dli_sname) return info.dli_sname;
    char buf[32];
    snprintf(buf, sizeof buf, "<kernel %p>", kern);
    return buf;
}
}  // namespace

void klog_record(const void *kern) {
    std::lock_guard<std::mutex> g(g_klog_mu);
    if (g_klog_on.load(std::memory_order_relaxed)) g_klog[kern]++;
}

std::string kernel_name_normalise(const char *name) {
    std::string s = name ? name : "";
    if (s.compare(0, 2, "_Z") == 0) {
        int st = 0;
        if (char *d = abi::__cxa_demangle(s.c_str(), nullptr, nullptr, &st)) {
            if (st == 0) s = d;
            free(d);
        }
    }
    erase_all(s, "(anonymous namespace)::");
    erase_all(s, "hx::");
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    int depth = 0;  // the parameter list: the first '(' outside the template arguments
    for (size_t i = 0; i < s.size(); i++) {
        if (s[i] == '<') depth++;
        else if (s[i] == '>') depth--;
        else if (s[i] == '(' && depth == 0) {
            s.erase(i);
            break;
        }
    }
    while (!s.empty() && s.back() == ' ') s.pop_back();
    return s;
}

}  // namespace hx

namespace {
int copy_out(const std::string &s, char *buf, uint64_t cap, uint64_t *needed) {
    if (needed) *needed = s.size() + 1;
    if (buf && cap) {
        const size_t n = std::min<size_t>(s.size(), cap - 1);
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (buf && cap > s.size()) || (!buf && !cap) ? HNSW_OK : HNSW_ERR_ARG;
}
}  // namespace

extern "C" {

int hnsw_kernel_log(int on) {
    std::lock_guard<std::mutex> g(hx::g_klog_mu);
    if (on) hx::g_klog.clear();
    hx::g_klog_on.store(on ? 1 : 0, std::memory_order_relaxed);
    return HNSW_OK;
}

int hnsw_kernel_log_get(char *buf, uint64_t cap, uint64_t *needed) {
    std::vector<std::pair<const void *, uint64_t>> items;
    {
        std::lock_guard<std::mutex> g(hx::g_klog_mu);
        items.assign(hx::g_klog.begin(), hx::g_klog.end());
    }
    std::map<std::string, uint64_t> named;  // (two pointers of one name, were there any, add up)
    for (const auto &it : items) named[hx::kernel_name_normalise(hx::raw_name(it.first).c_str())] += it.second;
    std::string out;
    for (const auto &kv : named) out += kv.first + " " + std::to_string(kv.second) + "\n";
    return copy_out(out, buf, cap, needed);
}

int hnsw_kernel_name(const char *name, char *buf, uint64_t cap, uint64_t *needed) {
    if (!name) return HNSW_ERR_ARG;
    return copy_out(hx::kernel_name_normalise(name), buf, cap, needed);
}

}  // extern "C"
