// row_table.cpp -- hnsw_row_table (row_table.h): the C entry points that manage a table of full rows in HBM, and the
// host's binary16 rounding, and the table's file.  Host logic only; the refinement and the boost that read the table are
// refine.cpp's, boost.cpp's and exact_scan.hip's.

#include "row_table.h"

#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "handle.h"

using hx::set_error;

static_assert(HX_ROWS_F32 == HNSW_ROWS_F32 && HX_ROWS_F16 == HNSW_ROWS_F16, "the kernel's dtypes are the ABI's");
static_assert(HX_REFINE_MAX_DIM == HNSW_REFINE_MAX_DIM, "the kernel's staged query holds the ABI's dimension limit");

hnsw_row_table::~hnsw_row_table() {
    if (d_rows) (void)hipFree(d_rows);
}

namespace hx {

uint16_t f16_from_f32(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7FFFFFFFu;
    if (x > 0x7F800000u) return sign | 0x7E00u;   // NaN
    if (x >= 0x477FF000u) return sign | 0x7C00u;  // 65520 (half way to 2^16, the even side) and beyond: +-inf
    if (x >= 0x38800000u) {                       // binary16's normal range, from 2^-14
        x -= 0x38000000u;                         // the exponent re-biased (127 -> 15)
        x += 0xFFFu + ((x >> 13) & 1u);           // to nearest, ties to even; a carry moves into the exponent
        return sign | (uint16_t)(x >> 13);
    }
    const uint32_t e = x >> 23;
    if (e < 102) return sign;  // below 2^-25: +-0 (2^-25 itself, e == 102, ties to the even 0 below)
    const uint32_t m = (x & 0x7FFFFFu) | 0x800000u, shift = 126 - e;  // the value in units of 2^-24 is m >> shift
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) r++;  // (0x400 is the smallest normal: the same bits)
    return sign | (uint16_t)r;
}

float f32_from_f16(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    uint32_t x;
    if (e == 0x1F) {
        x = sign | 0x7F800000u | (m << 13);
    } else if (e != 0) {
        x = sign | ((e + 112) << 23) | (m << 13);
    } else if (m == 0) {
        x = sign;
    } else {  // a subnormal: m * 2^-24, normal in f32
        const int top = 31 - __builtin_clz(m);  // 0 .. 9
        x = sign | ((uint32_t)(top + 103) << 23) | ((m << (23 - top)) & 0x7FFFFFu);
    }
    float f;
    memcpy(&f, &x, 4);
    return f;
}

}  // namespace hx

namespace {

int check_span(const char *what, const hnsw_row_table *t, uint64_t n, const void *buf) {
    if (!t || (n && !buf)) {
        set_error("row table: needs a table and %s", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

bool finite_f32(const float *v, uint64_t n, uint64_t *bad) {
    for (uint64_t i = 0; i < n; i++) {
        uint32_t x;
        memcpy(&x, v + i, 4);
        if ((x & 0x7F800000u) == 0x7F800000u) return *bad = i, false;
    }
    return true;
}

bool finite_f16(const uint16_t *v, uint64_t n, uint64_t *bad) {
    for (uint64_t i = 0; i < n; i++)
        if ((v[i] & 0x7C00u) == 0x7C00u) return *bad = i, false;
    return true;
}

int refuse_value(const hnsw_row_table *t, uint64_t first_id, uint64_t bad) {
    set_error("row table: row %llu holds a NaN or a value beyond the dtype's range; nothing is written",
              (unsigned long long)(first_id + bad / t->full_dim));
    return HNSW_ERR_NAN_INPUT;
}

// the device the table goes to at its first write: the handle's snapshot's, else the one the handle is bound to, else
// the calling thread's
int device_of(const hnsw_index *h, int *device) {
    if (h->dev.valid) return *device = h->dev.device, HNSW_OK;
    if (h->device >= 0) return *device = h->device, HNSW_OK;
    HIP_TRY(hipGetDevice(device));
    return HNSW_OK;
}

// n rows in the table's dtype, checked, to ids first_id .. first_id + n - 1 (mu held)
int store(hnsw_row_table *t, uint64_t first_id, uint64_t n, const void *src) {
    if (t->device < 0) {
        int device = -1;
        if (int rc = device_of(t->owner, &device)) return rc;
        t->device = device;
    }
    HIP_TRY(hipSetDevice(t->device));
    const uint64_t rb = t->row_bytes(), need = first_id + n;
    if (need > t->cap) {
        const uint64_t cap = std::max(need, t->cap + t->cap / 8);
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, cap * rb));
        if (t->rows) {
            const hipError_t e = hipMemcpy(p, t->d_rows, t->rows * rb, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) {
                (void)hipFree(p);
                set_error("row table: growing to %llu rows: %s", (unsigned long long)cap, hipGetErrorString(e));
                return HNSW_ERR_HIP;
            }
        }
        if (t->d_rows) (void)hipFree(t->d_rows);
        t->d_rows = p;
        t->cap = cap;
    }
    HIP_TRY(hipMemcpy(static_cast<unsigned char *>(t->d_rows) + first_id * rb, src, n * rb, hipMemcpyHostToDevice));
    t->rows = std::max(t->rows, need);
    t->owner->n_row_table_writes.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
}

// what both writes check before anything else (mu held)
int check_write(const hnsw_row_table *t, uint64_t first_id, uint64_t n) {
    if (first_id > t->rows) {
        set_error("row table: a write at id %llu would leave a hole behind its %llu rows", (unsigned long long)first_id,
                  (unsigned long long)t->rows);
        return HNSW_ERR_ARG;
    }
    if (n > 0xFFFFFFFFull - first_id) {
        set_error("row table: at most 2^32 - 1 rows");
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// ---- the table's file (hnsw_row_table_save / _load): big-endian like the index's own format (persist.cpp) ----
//   magic "HXRT" u32, version u32 = 1, full_dim u32, dtype u32, rows u64, then rows x full_dim elements of the dtype
constexpr uint32_t FILE_MAGIC = 0x48585254u, FILE_VERSION = 1;
constexpr size_t FILE_HEADER = 24;
constexpr uint64_t STAGE_BYTES = 64ull << 20;  // rows travel between HBM and the file in chunks of at most this

void put_be(uint8_t *p, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * (bytes - 1 - i)));
}
uint64_t get_be(const uint8_t *p, int bytes) {
    uint64_t v = 0;
    for (int i = 0; i < bytes; i++) v = (v << 8) | p[i];
    return v;
}
// n elements of es bytes between the host's order (little-endian) and the file's, in place
void swap_elements(uint8_t *p, uint64_t n, size_t es) {
    for (uint64_t i = 0; i < n; i++, p += es) std::reverse(p, p + es);
}
uint64_t chunk_rows(uint64_t row_bytes) { return std::max<uint64_t>(1, STAGE_BYTES / row_bytes); }
struct FileCloser {
    FILE *f;
    ~FileCloser() {
        if (f) fclose(f);
    }
};

}  // namespace

extern "C" {

int hnsw_f32_to_f16(const float *in, uint64_t n, uint16_t *out) {
    if (n && (!in || !out)) {
        set_error("f32 to f16: needs the values and a place for the halves");
        return HNSW_ERR_ARG;
    }
    for (uint64_t i = 0; i < n; i++)
        if ((hx::f16_from_f32(in[i]) & 0x7C00u) == 0x7C00u) {
            set_error("f32 to f16: value %llu is a NaN or rounds to an infinity; nothing is written", (unsigned long long)i);
            return HNSW_ERR_NAN_INPUT;
        }
    for (uint64_t i = 0; i < n; i++) out[i] = hx::f16_from_f32(in[i]);
    return HNSW_OK;
}

int hnsw_row_table_create(hnsw_index *h, uint32_t full_dim, uint32_t dtype, hnsw_row_table **out) {
    if (!h || !out) {
        set_error("row table: needs a handle and a place for the table");
        return HNSW_ERR_ARG;
    }
    if (full_dim == 0 || full_dim > HNSW_REFINE_MAX_DIM) {
        set_error("row table: needs 1 <= full_dim <= %d", HNSW_REFINE_MAX_DIM);
        return HNSW_ERR_ARG;
    }
    if (dtype != HNSW_ROWS_F32 && dtype != HNSW_ROWS_F16) {
        set_error("row table: the dtype is HNSW_ROWS_F32 (0) or HNSW_ROWS_F16 (1)");
        return HNSW_ERR_ARG;
    }
    hnsw_row_table *t = new (std::nothrow) hnsw_row_table();
    if (!t) return HNSW_ERR_OOM;
    t->owner = h;
    t->full_dim = full_dim;
    t->dtype = dtype;
    *out = t;
    return HNSW_OK;
}

void hnsw_row_table_free(hnsw_row_table *t) { delete t; }

int hnsw_row_table_info(const hnsw_row_table *t, uint32_t *full_dim, uint32_t *dtype, uint64_t *rows) {
    if (!t) {
        set_error("row table: needs a table");
        return HNSW_ERR_ARG;
    }
    if (full_dim) *full_dim = t->full_dim;
    if (dtype) *dtype = t->dtype;
    if (rows) *rows = t->rows;
    return HNSW_OK;
}

int hnsw_row_table_write(hnsw_row_table *t, uint64_t first_id, uint64_t n, const float *rows) {
    if (int rc = check_span("the rows to write", t, n, rows)) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if (int rc = check_write(t, first_id, n)) return rc;
    if (n == 0) return HNSW_OK;
    const uint64_t total = n * t->full_dim;
    uint64_t bad = 0;
    if (t->dtype == HNSW_ROWS_F32) {
        if (!finite_f32(rows, total, &bad)) return refuse_value(t, first_id, bad);
        return store(t, first_id, n, rows);
    }
    std::vector<uint16_t> halves;
    try {
        halves.resize(total);
    } catch (const std::bad_alloc &) {
        set_error("row table: out of memory for %llu rows of halves", (unsigned long long)n);
        return HNSW_ERR_OOM;
    }
    for (uint64_t i = 0; i < total; i++) halves[i] = hx::f16_from_f32(rows[i]);
    if (!finite_f16(halves.data(), total, &bad)) return refuse_value(t, first_id, bad);
    return store(t, first_id, n, halves.data());
}

int hnsw_row_table_write_raw(hnsw_row_table *t, uint64_t first_id, uint64_t n, const void *rows) {
    if (int rc = check_span("the rows to write", t, n, rows)) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if (int rc = check_write(t, first_id, n)) return rc;
    if (n == 0) return HNSW_OK;
    const uint64_t total = n * t->full_dim;
    uint64_t bad = 0;
    const bool fine = t->dtype == HNSW_ROWS_F32 ? finite_f32(static_cast<const float *>(rows), total, &bad)
                                                : finite_f16(static_cast<const uint16_t *>(rows), total, &bad);
    if (!fine) return refuse_value(t, first_id, bad);
    return store(t, first_id, n, rows);
}

int hnsw_row_table_read(hnsw_row_table *t, uint64_t first_id, uint64_t n, float *out) {
    if (int rc = check_span("a place for the rows", t, n, out)) return rc;
    std::lock_guard<std::mutex> g(t->mu);
    if (first_id > t->rows || n > t->rows - first_id) {
        set_error("row table: rows %llu .. %llu of %llu", (unsigned long long)first_id, (unsigned long long)(first_id + n),
                  (unsigned long long)t->rows);
        return HNSW_ERR_ARG;
    }
    if (n == 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(t->device));
    const uint64_t rb = t->row_bytes(), total = n * t->full_dim;
    const unsigned char *src = static_cast<const unsigned char *>(t->d_rows) + first_id * rb;
    if (t->dtype == HNSW_ROWS_F32) {
        HIP_TRY(hipMemcpy(out, src, n * rb, hipMemcpyDeviceToHost));
        return HNSW_OK;
    }
    std::vector<uint16_t> halves;
    try {
        halves.resize(total);
    } catch (const std::bad_alloc &) {
        set_error("row table: out of memory for %llu rows of halves", (unsigned long long)n);
        return HNSW_ERR_OOM;
    }
    HIP_TRY(hipMemcpy(halves.data(), src, n * rb, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < total; i++) out[i] = hx::f32_from_f16(halves[i]);
    return HNSW_OK;
}

int hnsw_row_table_device(const hnsw_row_table *t, const void **d_ptr, uint64_t *rows) {
    if (!t || !d_ptr) {
        set_error("row table: needs a table and a place for the pointer");
        return HNSW_ERR_ARG;
    }
    *d_ptr = t->d_rows;
    if (rows) *rows = t->rows;
    return HNSW_OK;
}

int hnsw_row_table_save(hnsw_row_table *t, const char *path) {
    if (!t || !path) {
        set_error("row table: saving needs a table and a path");
        return HNSW_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(t->mu);
    FILE *f = fopen(path, "wb");
    if (!f) {
        set_error("row table: could not create %s", path);
        return HNSW_ERR_IO;
    }
    FileCloser closer{f};
    uint8_t head[FILE_HEADER];
    put_be(head, FILE_MAGIC, 4), put_be(head + 4, FILE_VERSION, 4), put_be(head + 8, t->full_dim, 4);
    put_be(head + 12, t->dtype, 4), put_be(head + 16, t->rows, 8);
    bool ok = fwrite(head, 1, FILE_HEADER, f) == FILE_HEADER;
    if (t->rows) {  // (a table that was never written touches no device)
        HIP_TRY(hipSetDevice(t->device));
        const uint64_t rb = t->row_bytes(), per = chunk_rows(rb);
        const size_t es = t->dtype == HNSW_ROWS_F16 ? 2 : 4;
        std::vector<uint8_t> stage;
        try {
            stage.resize(std::min(per, t->rows) * rb);
        } catch (const std::bad_alloc &) {
            set_error("row table: out of memory for the staging of %s", path);
            return HNSW_ERR_OOM;
        }
        for (uint64_t r0 = 0; ok && r0 < t->rows; r0 += per) {
            const uint64_t n = std::min(per, t->rows - r0);
            HIP_TRY(hipMemcpy(stage.data(), static_cast<const unsigned char *>(t->d_rows) + r0 * rb, n * rb,
                              hipMemcpyDeviceToHost));
            swap_elements(stage.data(), n * t->full_dim, es);
            ok = fwrite(stage.data(), 1, n * rb, f) == n * rb;
        }
    }
    closer.f = nullptr;
    if (fclose(f) != 0 || !ok) {
        set_error("row table: could not write %s", path);
        return HNSW_ERR_IO;
    }
    return HNSW_OK;
}

int hnsw_row_table_load(hnsw_index *h, const char *path, hnsw_row_table **out) {
    if (!h || !path || !out) {
        set_error("row table: loading needs a handle, a path and a place for the table");
        return HNSW_ERR_ARG;
    }
    FILE *f = fopen(path, "rb");
    if (!f) {
        set_error("row table: could not open %s", path);
        return HNSW_ERR_IO;
    }
    FileCloser closer{f};
    auto corrupt = [&](const char *why) {
        set_error("row table: %s: %s", path, why);
        return HNSW_ERR_IO;
    };
    uint8_t head[FILE_HEADER];
    if (fread(head, 1, FILE_HEADER, f) != FILE_HEADER) return corrupt("shorter than its header");
    if (get_be(head, 4) != FILE_MAGIC) return corrupt("not a row table (magic)");
    if (get_be(head + 4, 4) != FILE_VERSION) return corrupt("a version this library does not read");
    const uint64_t full_dim = get_be(head + 8, 4), dtype = get_be(head + 12, 4), rows = get_be(head + 16, 8);
    if (full_dim == 0 || full_dim > HNSW_REFINE_MAX_DIM) return corrupt("full_dim out of range");
    if (dtype != HNSW_ROWS_F32 && dtype != HNSW_ROWS_F16) return corrupt("an unknown dtype");
    if (rows > 0xFFFFFFFFull) return corrupt("more than 2^32 - 1 rows");
    const uint64_t rb = full_dim * (dtype == HNSW_ROWS_F16 ? 2 : 4);
    struct stat st;
    if (fstat(fileno(f), &st) != 0 || (uint64_t)st.st_size != FILE_HEADER + rows * rb)
        return corrupt("its length is not what its header says");
    hnsw_row_table *t = nullptr;
    if (int rc = hnsw_row_table_create(h, (uint32_t)full_dim, (uint32_t)dtype, &t)) return rc;
    auto fail = [&](int rc) {
        delete t;
        return rc;
    };
    if (rows) {
        const uint64_t per = chunk_rows(rb);
        const size_t es = dtype == HNSW_ROWS_F16 ? 2 : 4;
        std::vector<uint8_t> stage;
        try {
            stage.resize(std::min(per, rows) * rb);
        } catch (const std::bad_alloc &) {
            set_error("row table: out of memory for the staging of %s", path);
            return fail(HNSW_ERR_OOM);
        }
        for (uint64_t r0 = 0; r0 < rows; r0 += per) {  // (nobody else has the table yet: no lock)
            const uint64_t n = std::min(per, rows - r0), total = n * full_dim;
            if (fread(stage.data(), 1, n * rb, f) != n * rb) return fail(corrupt("could not be read"));
            swap_elements(stage.data(), total, es);
            uint64_t bad = 0;
            const bool fine = dtype == HNSW_ROWS_F32 ? finite_f32(reinterpret_cast<const float *>(stage.data()), total, &bad)
                                                     : finite_f16(reinterpret_cast<const uint16_t *>(stage.data()), total, &bad);
            if (!fine) return fail(corrupt("holds a NaN or an infinity"));
            if (int rc = store(t, r0, n, stage.data())) return fail(rc);
        }
    }
    *out = t;
    return HNSW_OK;
}

}  // extern "C"
