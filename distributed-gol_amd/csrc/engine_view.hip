// engine_view.hip -- windowed access to the resident board: a rectangle of it as bytes, out
// (golhip_store_rect) and in (golhip_load_rect, a change to the RUNNING board: the turn is kept),
// and the density viewport (golhip_view_counts / golhip_view).  Kernels: view_kernels.hip.
//
// Reference roles: sdl/loop.go (the window showing the world, the `s` key's PGM) -> a window of
// the board at a zoom, instead of the 4 GiB PGM of a 65536^2 board; gol/io.go:42-128 moves the
// whole world, these calls only the rectangle asked for.
//
// Rows: the rectangle's rows [y, y + R) wrap mod height, and each strip of the handle holds an
// interval of rows, so per strip the rectangle is at most two intervals (two when it wraps past
// the strip): row_spans().  Every call stages through Shard::stage in chunks: none allocates or
// frees device memory.
#include <algorithm>
#include <cstring>

#include "golhip_engine.hpp"

namespace golhip {
namespace {

// Rows [rr, rr + n) of the rectangle are local rows [local, local + n) of shard s.
struct Span {
    Shard *s;
    int64_t rr, n, local;
};

std::vector<Span> row_spans(golhip_t h, int64_t y0, int64_t R) {
    std::vector<Span> out;
    for (auto &s : h->shards)
        for (int m = 0; m < 2; ++m) {  // the strip, and its image one torus height further down
            const int64_t lo = std::max(y0, s.y0 + m * h->height);
            const int64_t hi = std::min(y0 + R, s.y0 + s.rows + m * h->height);
            if (lo < hi) out.push_back({&s, lo - y0, hi - lo, lo - m * h->height - s.y0});
        }
    return out;
}

bool holds_every_row(golhip_t h) {
    int64_t rows = 0;
    for (auto &s : h->shards) rows += s.rows;
    return rows == h->height;
}

int64_t mod_floor(int64_t a, int64_t m) {
    const int64_t r = a % m;
    return r < 0 ? r + m : r;
}

int check_rect(golhip_t h, int64_t w, int64_t hgt) {
    if (w < 1 || w > h->width)
        return fail(h, GOLHIP_ERR_ARG, "w %lld is outside 1..%lld (the board's width)", (long long)w,
                    (long long)h->width);
    if (hgt < 1 || hgt > h->height)
        return fail(h, GOLHIP_ERR_ARG, "hgt %lld is outside 1..%lld (the board's height)", (long long)hgt,
                    (long long)h->height);
    return GOLHIP_OK;
}

// Host <-> device bytes of the rectangle, in row chunks through each strip's stage.
int transfer_rect(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, uint8_t *host, size_t row_stride,
                  bool to_device, int mode) {
    const int64_t x0 = mod_floor(x, h->width), y0 = mod_floor(y, h->height);
    if (!to_device && !holds_every_row(h))  // rows of other ranks read as dead
        for (int64_t r = 0; r < hgt; ++r) std::memset(host + (size_t)r * row_stride, 0, (size_t)w);
    for (const Span &sp : row_spans(h, y0, hgt)) {
        Shard &s = *sp.s;
        HIPCHK(h, hipSetDevice(s.device));
        const int64_t cr = std::max<int64_t>(1, s.stage_bytes / w);
        for (int64_t yy = 0; yy < sp.n; yy += cr) {
            const int64_t nr = std::min(cr, sp.n - yy);
            uint32_t *rows_dev = h->row0(s, h->cur) + (sp.local + yy) * h->pitch;
            uint8_t *hrows = host + (size_t)(sp.rr + yy) * row_stride;
            if (to_device) {
                HIPCHK(h, hipMemcpy2DAsync(s.stage, (size_t)w, hrows, row_stride, (size_t)w, (size_t)nr,
                                           hipMemcpyHostToDevice, s.compute));
                HIPCHK(h, launch_rect_pack(s.stage, nr, h->width, h->wd, x0, w, mode, rows_dev, h->pitch, s.compute));
            } else {
                HIPCHK(h, launch_rect_unpack(rows_dev, h->pitch, nr, h->wd, x0, w, s.stage, s.compute));
                HIPCHK(h, hipMemcpy2DAsync(hrows, row_stride, s.stage, (size_t)w, (size_t)w, (size_t)nr,
                                           hipMemcpyDeviceToHost, s.compute));
            }
            SYNCCHK(h, s.compute);
        }
    }
    return GOLHIP_OK;
}

int check_view(golhip_t h, int64_t w, int64_t hgt, int scale) {
    if (scale < 1 || scale > 1024 || (scale & (scale - 1)))
        return fail(h, GOLHIP_ERR_ARG, "scale %d is not a power of two in 1..1024", scale);
    int rc = check_rect(h, w, hgt);
    if (rc) return rc;
    if (w * scale > h->width)
        return fail(h, GOLHIP_ERR_ARG, "w * scale = %lld * %d exceeds the board's width %lld", (long long)w, scale,
                    (long long)h->width);
    if (hgt * scale > h->height)
        return fail(h, GOLHIP_ERR_ARG, "hgt * scale = %lld * %d exceeds the board's height %lld", (long long)hgt,
                    scale, (long long)h->height);
    return GOLHIP_OK;
}

// The counts of the w x hgt viewport into out (dense).  Per strip interval, pixel rows and pixel
// columns are chunked to the stage (uint32 per pixel); a pixel row cut by a strip boundary or by
// the row wrap comes back as partial counts from each side and is summed here.
int view_counts_impl(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, int scale, uint32_t *out) {
    const int64_t x0 = mod_floor(x, h->width), y0 = mod_floor(y, h->height);
    const std::vector<Span> spans = row_spans(h, y0, hgt * scale);
    // direct: every launch's pixel rows are whole, so its image is copied straight into `out`
    bool direct = holds_every_row(h);
    for (const Span &sp : spans) direct = direct && sp.rr % scale == 0 && sp.n % scale == 0;
    std::vector<uint32_t> part;
    if (!direct) std::memset(out, 0, sizeof(uint32_t) * (size_t)(w * hgt));
    for (const Span &sp : spans) {
        Shard &s = *sp.s;
        HIPCHK(h, hipSetDevice(s.device));
        uint32_t *stage = reinterpret_cast<uint32_t *>(s.stage);
        const int64_t cap = std::max<int64_t>(1, s.stage_bytes / (int64_t)sizeof(uint32_t));
        const int64_t cw = std::min(w, cap), cpr = std::max<int64_t>(1, cap / cw);
        const int64_t phase = sp.rr % scale, p0 = sp.rr / scale, npr = (phase + sp.n + scale - 1) / scale;
        for (int64_t pc = 0; pc < npr; pc += cpr) {
            const int64_t np = std::min(cpr, npr - pc);
            const int64_t lr = std::max<int64_t>(0, pc * scale - phase);
            const int64_t le = std::min(sp.n, (pc + np) * scale - phase);
            const uint32_t *rows_dev = h->row0(s, h->cur) + (sp.local + lr) * h->pitch;
            for (int64_t ci = 0; ci < w; ci += cw) {
                const int64_t nc = std::min(cw, w - ci);
                HIPCHK(h, launch_view_counts(rows_dev, h->pitch, le - lr, (int32_t)(pc == 0 ? phase : 0), h->wd,
                                             (x0 + ci * scale) % h->width, scale, (int32_t)nc, np, stage, s.compute));
                uint32_t *dst = out + (p0 + pc) * w + ci;
                if (direct) {
                    HIPCHK(h, hipMemcpy2DAsync(dst, sizeof(uint32_t) * (size_t)w, stage, sizeof(uint32_t) * (size_t)nc,
                                               sizeof(uint32_t) * (size_t)nc, (size_t)np, hipMemcpyDeviceToHost,
                                               s.compute));
                    SYNCCHK(h, s.compute);
                    continue;
                }
                part.resize((size_t)(np * nc));
                HIPCHK(h, hipMemcpyAsync(part.data(), stage, sizeof(uint32_t) * part.size(), hipMemcpyDeviceToHost,
                                         s.compute));
                SYNCCHK(h, s.compute);
                for (int64_t j = 0; j < np; ++j)
                    for (int64_t i = 0; i < nc; ++i) dst[j * w + i] += part[(size_t)(j * nc + i)];
            }
        }
    }
    return GOLHIP_OK;
}

}  // namespace
}  // namespace golhip

using namespace golhip;

// ================================================================================ C ABI ====
extern "C" {

int golhip_store_rect(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, uint8_t *out, size_t row_stride) {
    if (!h) return GOLHIP_ERR_ARG;
    int rc = check_rect(h, w, hgt);
    if (rc) return rc;
    if (!out) return fail(h, GOLHIP_ERR_ARG, "out is null");
    if (row_stride < (size_t)w)
        return fail(h, GOLHIP_ERR_ARG, "row_stride %zu < w %lld", row_stride, (long long)w);
    if ((rc = sync_all(h))) return rc;
    return transfer_rect(h, x, y, w, hgt, out, row_stride, false, 0);
}

int golhip_load_rect(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, const uint8_t *cells,
                     size_t row_stride, int mode) {
    if (!h) return GOLHIP_ERR_ARG;
    int rc = check_rect(h, w, hgt);
    if (rc) return rc;
    if (!cells) return fail(h, GOLHIP_ERR_ARG, "cells is null");
    if (row_stride < (size_t)w)
        return fail(h, GOLHIP_ERR_ARG, "row_stride %zu < w %lld", row_stride, (long long)w);
    if (mode < 0 || mode > 2) return fail(h, GOLHIP_ERR_ARG, "mode %d is outside 0..2", mode);
    if ((rc = sync_all(h))) return rc;
    // whatever was derived from the old cells is stale from here on, also when a chunk fails: the
    // previous generation (golhip_flips), the last flips board, the stable-slab flags.  The turn,
    // the buffers and their parity stay: captured graphs remain valid, and the halos are
    // re-exchanged at the start of the next block as after golhip_load_bytes
    h->prev_valid = false;
    h->diff_valid = false;
    h->act_valid = false;
    return transfer_rect(h, x, y, w, hgt, const_cast<uint8_t *>(cells), row_stride, true, mode);
}

int golhip_view_counts(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, int scale, uint32_t *out) {
    if (!h) return GOLHIP_ERR_ARG;
    int rc = check_view(h, w, hgt, scale);
    if (rc) return rc;
    if (!out) return fail(h, GOLHIP_ERR_ARG, "out is null");
    if ((rc = sync_all(h))) return rc;
    return view_counts_impl(h, x, y, w, hgt, scale, out);
}

int golhip_view(golhip_t h, int64_t x, int64_t y, int64_t w, int64_t hgt, int scale, uint8_t *out,
                size_t row_stride) {
    if (!h) return GOLHIP_ERR_ARG;
    int rc = check_view(h, w, hgt, scale);
    if (rc) return rc;
    if (!out) return fail(h, GOLHIP_ERR_ARG, "out is null");
    if (row_stride < (size_t)w)
        return fail(h, GOLHIP_ERR_ARG, "row_stride %zu < w %lld", row_stride, (long long)w);
    if (!holds_every_row(h))
        return fail(h, GOLHIP_ERR_STATE,
                    "this handle holds rows [%lld, %lld) of %lld: a partial count has no grey value "
                    "(sum golhip_view_counts over the ranks)",
                    (long long)h->shards.front().y0, (long long)(h->shards.back().y0 + h->shards.back().rows),
                    (long long)h->height);
    if ((rc = sync_all(h))) return rc;
    std::vector<uint32_t> counts((size_t)(w * hgt));
    if ((rc = view_counts_impl(h, x, y, w, hgt, scale, counts.data()))) return rc;
    const uint64_t cells = (uint64_t)scale * (uint64_t)scale;
    for (int64_t j = 0; j < hgt; ++j)
        for (int64_t i = 0; i < w; ++i)
            out[(size_t)j * row_stride + (size_t)i] =
                (uint8_t)(((uint64_t)counts[(size_t)(j * w + i)] * 255 + cells - 1) / cells);
    return GOLHIP_OK;
}

}  // extern "C"
