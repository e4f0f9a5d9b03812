// snapshot.cpp -- snapshot replication behind hnsw_snapshot_describe / _adopt / _commit: the 32-word header that travels
// in hnsw_snapshot_desc.header, a live snapshot described by it, and an empty handle made a device-only replica from it.

#include <algorithm>
#include <cstring>

#include "handle.h"

namespace hx {

namespace {

struct SnapHeader {  // what travels in hnsw_snapshot_desc.header (32 words)
    uint32_t magic, version;
    int32_t kind;
    uint32_t dim, n_points, nb_layers, ep, S0, S1, row_stride, half_bytes, nch4, rem;
    uint32_t fat_stride_lo, fat_stride_hi;
    uint32_t m, ef_cons;
    uint32_t flags;  // bit 0: the cosine option (queries are normalised on arrival)
    uint32_t reserved[14];
};
static_assert(sizeof(SnapHeader) == 32 * 4, "snapshot header is 32 words");
constexpr uint32_t SNAP_MAGIC = 0x48584E53u;  // "SNXH"

// The scalars a header and a DevView share, listed once: either direction hands in the assignment it wants,
// move(header's field, view's field).  (fat_stride, one 64-bit value in two words, is spelled out by each direction.)
template <class Header, class View, class Move>
void each_scalar(Header &hd, View &v, Move move) {
    move(hd.kind, v.kind), move(hd.dim, v.dim), move(hd.n_points, v.n_points), move(hd.nb_layers, v.nb_layers);
    move(hd.ep, v.ep), move(hd.S0, v.S0), move(hd.S1, v.S1), move(hd.row_stride, v.row_stride);
    move(hd.half_bytes, v.half_bytes), move(hd.nch4, v.nch4), move(hd.rem, v.rem);
}

}  // namespace

int snapshot_describe(hnsw_index *h, hnsw_snapshot_desc *out) {
    int rc = ensure_uploaded(h);
    if (rc != HNSW_OK) return rc;
    memset(out, 0, sizeof(*out));
    h->dev.describe(out->bytes, out->ptr);
    SnapHeader hd{SNAP_MAGIC, 1};  // (the rest zero)
    const DevView &v = h->dev.view;
    each_scalar(hd, v, [](auto &in_header, const auto &in_view) { in_header = in_view; });
    hd.fat_stride_lo = (uint32_t)v.fat_stride, hd.fat_stride_hi = (uint32_t)(v.fat_stride >> 32);
    hd.m = (uint32_t)h->host->params.m, hd.ef_cons = (uint32_t)h->host->params.ef_cons;
    hd.flags = h->cosine ? 1u : 0u;
    memcpy(out->header, &hd, sizeof(hd));
    return HNSW_OK;
}

int snapshot_adopt(hnsw_index *h, hnsw_snapshot_desc *d) {
    SnapHeader hd;
    memcpy(&hd, d->header, sizeof(hd));
    if (hd.magic != SNAP_MAGIC || hd.version != 1) {
        set_error("hnsw_snapshot_adopt: not a snapshot header");
        return HNSW_ERR_ARG;
    }
    if (h->host->len() != 0 || is_replica(h)) {
        set_error("hnsw_snapshot_adopt: the receiving handle must be empty (fresh from hnsw_create)");
        return HNSW_ERR_ARG;
    }
    if (hd.kind != h->host->kind || hd.dim != h->host->dim || hd.m != (uint32_t)h->host->params.m) {
        set_error("hnsw_snapshot_adopt: snapshot of a %ud kind-%d m=%u index offered to a %ud kind-%d m=%u handle", hd.dim,
                  hd.kind, hd.m, h->host->dim, h->host->kind, (uint32_t)h->host->params.m);
        return HNSW_ERR_BAD_DIM;
    }
    // Every stride in the header is recomputed from the receiving handle's own m, dim and kind and must agree (the
    // kernels index the arrays by id without a range check, and a zero stride must never reach a division), then
    // the array sizes must be what the header implies.
    const bool q8 = h->host->kind == HNSW_VEC_QUANT8;
    const uint32_t half = q8 ? quant_half_bytes(hd.dim) : 0, stride = q8 ? 2 * half : f32_row_stride(hd.dim);
    const uint32_t S0 = adj_stride(h->host->layer_m(0), 32), S1 = adj_stride(h->host->params.m, 8);
    const uint64_t fat_stride = ((uint64_t)hd.fat_stride_hi << 32) | hd.fat_stride_lo;
    if (hd.S0 != S0 || hd.S1 != S1 || hd.row_stride != stride || hd.half_bytes != half || hd.nch4 != 4 * (hd.dim / 8) ||
        hd.rem != hd.dim % 8 || (fat_stride != 0 && fat_stride != (uint64_t)S0 * stride)) {
        set_error("hnsw_snapshot_adopt: the header's strides are not those of a %ud kind-%d m=%u index", hd.dim, hd.kind, hd.m);
        return HNSW_ERR_ARG;
    }
    const uint64_t N = hd.n_points;
    if (N == 0 || N > 0x7FFFFFFFull || d->bytes[0] != N * stride || d->bytes[1] != N * S0 * 4ull || d->bytes[3] != N * 4ull ||
        d->bytes[2] == 0 || d->bytes[2] % (S1 * 4ull) != 0 || d->bytes[4] < 4 || d->bytes[4] % 4 != 0 || d->bytes[5] < 4 ||
        (d->bytes[6] != 0) != (fat_stride != 0) || (fat_stride != 0 && d->bytes[6] != N * fat_stride) || hd.ep >= N ||
        hd.nb_layers == 0) {
        set_error("hnsw_snapshot_adopt: array sizes do not match the header");
        return HNSW_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(h->mu);
    void *pp[HNSW_SNAPSHOT_ARRAYS];
    int rc = h->dev.adopt_alloc(h->device, d->bytes, pp);
    if (rc != HNSW_OK) {
        h->dev.release();
        return rc;
    }
    h->device = h->dev.device;
    std::copy(pp, pp + HNSW_SNAPSHOT_ARRAYS, d->ptr);
    DevView v{};
    each_scalar(hd, v, [](const auto &in_header, auto &in_view) { in_view = in_header; });
    v.fat_stride = fat_stride;
    h->dev.view = v;  // scalars now, pointers at commit
    h->dev.replica = true;
    h->cosine = (hd.flags & 1u) != 0;
    return HNSW_OK;
}

int snapshot_commit(hnsw_index *h) {
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->dev.replica || h->dev.valid) {
        set_error("hnsw_snapshot_commit: no adopted snapshot waiting");
        return HNSW_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(h->dev.device));
    HIP_TRY(hipDeviceSynchronize());  // whatever filled the arrays has finished
    h->dev.adopt_commit(h->dev.view);
    h->host->params.ep = h->dev.view.ep;
    return HNSW_OK;
}

}  // namespace hx
