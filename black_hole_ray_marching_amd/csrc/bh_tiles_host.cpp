// bh_tiles_host.cpp — shards and packed tiles on the host (include/bh_render.h): tile counts and sizes, the
// unpack launches (bh_tiles.hip) and the weighted partitions.
#include <atomic>
#include <new>

#include "bh_host.hpp"

static std::atomic<uint64_t> g_partition_serial{0};

extern "C" {

int64_t bh_shard_tile_count(uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count) {
    if (width == 0 || height == 0 || shard_count == 0 || shard_index >= shard_count) return bad_arg(__func__, __LINE__);
    return (int64_t)bh::shard_tile_count((width + 7u) / 8u, (height + 7u) / 8u, shard_index, shard_count);
}

int bh_tiles_unpack(const void* packed, void* out, uint32_t width, uint32_t height, uint32_t shard_count,
                    uint64_t shard_stride_tiles, uint32_t bpp, void* stream) {
    if (!packed || !out || width == 0 || height == 0 || shard_count == 0) return bad_arg(__func__, __LINE__);
    if (bpp != 4 && bpp != 8 && bpp != 16) return bad_arg(__func__, __LINE__);
    for (uint32_t k = 0; k < shard_count; ++k)
        if (bh::shard_tile_count((width + 7u) / 8u, (height + 7u) / 8u, k, shard_count) > shard_stride_tiles)
            return bad_arg(__func__, __LINE__);
    int e = bh_launch_tiles_unpack(packed, out, width, height, shard_count, shard_stride_tiles, bpp,
                                   reinterpret_cast<hipStream_t>(stream));
    if (e != 0) return hip_fail((hipError_t)e, "tiles unpack launch");
    return BH_OK;
}

// an RGBM unpack's format: a bh_out_format, or BH_OUT_RGBA16F | BH_UNPACK_RGBM14
static bool unpack_format_ok(uint32_t format) {
    return format <= BH_OUT_BGRA8_SRGB || format == (BH_OUT_RGBA16F | BH_UNPACK_RGBM14);
}

int bh_tiles_unpack_rgb_rows(const void* packed, void* out, uint32_t width, uint32_t height, uint32_t shard_count,
                             uint64_t shard_stride_tiles, uint32_t format, uint32_t rows_in_flight, void* stream) {
    if (!packed || !out || width == 0 || height == 0 || shard_count == 0) return bad_arg(__func__, __LINE__);
    if (format > BH_OUT_BGRA8_SRGB) return bad_arg(__func__, __LINE__);
    for (uint32_t k = 0; k < shard_count; ++k)
        if (bh::shard_tile_count((width + 7u) / 8u, (height + 7u) / 8u, k, shard_count) > shard_stride_tiles)
            return bad_arg(__func__, __LINE__);
    int e = bh_launch_tiles_unpack_rgb(packed, out, width, height, shard_count, shard_stride_tiles, format,
                                       rows_in_flight, reinterpret_cast<hipStream_t>(stream));
    if (e != 0) return hip_fail((hipError_t)e, "tiles unpack launch");
    return BH_OK;
}

int bh_tiles_unpack_rgb(const void* packed, void* out, uint32_t width, uint32_t height, uint32_t shard_count,
                        uint64_t shard_stride_tiles, uint32_t format, void* stream) {
    return bh_tiles_unpack_rgb_rows(packed, out, width, height, shard_count, shard_stride_tiles, format, 0u, stream);
}

int bh_tiles_unpack_rgbm(const void* packed, void* out, void* out_bo, uint32_t width, uint32_t height,
                         uint32_t shard_count, uint64_t shard_stride_tiles, uint32_t format, uint32_t rows_in_flight,
                         void* stream) {
    if (!packed || !out || width == 0 || height == 0 || shard_count == 0) return bad_arg(__func__, __LINE__);
    if (!unpack_format_ok(format)) return bad_arg(__func__, __LINE__);
    for (uint32_t k = 0; k < shard_count; ++k)
        if (bh::shard_tile_count((width + 7u) / 8u, (height + 7u) / 8u, k, shard_count) > shard_stride_tiles)
            return bad_arg(__func__, __LINE__);
    int e = bh_launch_tiles_unpack_rgbm(packed, out, out_bo, width, height, shard_count, shard_stride_tiles, nullptr,
                                        format, rows_in_flight, reinterpret_cast<hipStream_t>(stream));
    if (e != 0) return hip_fail((hipError_t)e, "tiles unpack launch");
    return BH_OK;
}

namespace {
// Owner of each residue (tx + 3 ty) mod M, M = sum(weights): smooth weighted round robin, so each shard's
// residues are spread evenly over the M.  Empty if the weights are unusable.
std::vector<uint32_t> partition_owners(uint32_t S, const uint32_t* w) {
    uint64_t M = 0;
    for (uint32_t k = 0; k < S; ++k) M += w[k];
    if (M == 0 || M > 4096) return {};
    std::vector<uint32_t> owner(M);
    std::vector<int64_t> cw(S, 0);
    for (uint64_t v = 0; v < M; ++v) {
        uint32_t best = 0;
        for (uint32_t k = 0; k < S; ++k) {
            cw[k] += w[k];
            if (cw[k] > cw[best]) best = k;
        }
        owner[v] = best;
        cw[best] -= (int64_t)M;
    }
    return owner;
}
}  // namespace

int bh_partition_map(uint32_t width, uint32_t height, uint32_t S, const uint32_t* weights, uint32_t* owner_out,
                     uint32_t* index_out) {
    if (width == 0 || height == 0 || width > 65536u || height > 65536u || S == 0 || S > 256 || !weights)
        return bad_arg(__func__, __LINE__);
    const std::vector<uint32_t> owner = partition_owners(S, weights);
    if (owner.empty()) return bad_arg(__func__, __LINE__);
    const uint32_t M = (uint32_t)owner.size(), tx_n = (width + 7u) / 8u, ty_n = (height + 7u) / 8u;
    std::vector<uint32_t> next(S, 0);
    for (uint32_t ty = 0; ty < ty_n; ++ty)
        for (uint32_t tx = 0; tx < tx_n; ++tx) {
            const uint32_t k = owner[(tx + 3ull * ty) % M];
            const size_t t = (size_t)ty * tx_n + tx;
            if (owner_out) owner_out[t] = k;
            if (index_out) index_out[t] = next[k];
            ++next[k];
        }
    return BH_OK;
}

int bh_partition_create(uint32_t width, uint32_t height, uint32_t S, const uint32_t* weights, int device,
                        bh_partition** out) {
    if (!out) return bad_arg(__func__, __LINE__);
    *out = nullptr;
    const uint32_t tx_n = (width + 7u) / 8u, ty_n = (height + 7u) / 8u;
    const size_t n = (size_t)tx_n * ty_n;
    if (n >= (1u << 24)) return bad_arg(__func__, __LINE__);  // packed indices carry 24 bits
    std::vector<uint32_t> owner(n), index(n);
    int st = bh_partition_map(width, height, S, weights, owner.data(), index.data());
    if (st != BH_OK) return st;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return BH_ERR_NO_DEVICE;
    bh_partition* P = new (std::nothrow) bh_partition;
    if (!P) return BH_ERR_OUT_OF_MEMORY;
    P->width = width; P->height = height; P->shard_count = S; P->tiles_x = tx_n; P->tiles_y = ty_n;
    P->device = device;
    P->serial = ++g_partition_serial;
    P->count.assign(S, 0);
    for (size_t t = 0; t < n; ++t) ++P->count[owner[t]];
    P->offset.assign(S, 0);
    for (uint32_t k = 1; k < S; ++k) P->offset[k] = P->offset[k - 1] + P->count[k - 1];
    std::vector<uint32_t> list(n), loc(n);
    for (size_t t = 0; t < n; ++t) {
        const uint32_t k = owner[t];
        list[P->offset[k] + index[t]] = (uint32_t)(t % tx_n) | (uint32_t)(t / tx_n) << 16;
        loc[t] = index[t] | k << 24;
    }
    DeviceScope dev(device);
    hipError_t e = dev.err;
    if (e != hipSuccess || (e = hipMalloc(&P->tile_list, n * 4)) != hipSuccess || (e = hipMalloc(&P->tile_loc, n * 4)) != hipSuccess ||
        (e = hipMemcpy(P->tile_list, list.data(), n * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(P->tile_loc, loc.data(), n * 4, hipMemcpyHostToDevice)) != hipSuccess) {
        st = alloc_fail(e, "partition tables");
        if (P->tile_list) (void)hipFree(P->tile_list);
        if (P->tile_loc) (void)hipFree(P->tile_loc);
        delete P;
        return st;
    }
    *out = P;
    return BH_OK;
}

int bh_partition_destroy(bh_partition* P) {
    if (!P) return BH_OK;
    {
        DeviceScope dev(P->device);
        if (P->tile_list) (void)hipFree(P->tile_list);
        if (P->tile_loc) (void)hipFree(P->tile_loc);
    }
    delete P;
    return BH_OK;
}

int64_t bh_partition_tile_count(const bh_partition* P, uint32_t shard_index) {
    if (!P || shard_index >= P->shard_count) return bad_arg(__func__, __LINE__);
    return P->count[shard_index];
}

int bh_tiles_unpack_rgbm_partition(const void* packed, void* out, void* out_bo, const bh_partition* P,
                                   uint64_t shard_stride_tiles, uint32_t format, uint32_t rows_in_flight,
                                   void* stream) {
    if (!packed || !out || !P || !unpack_format_ok(format)) return bad_arg(__func__, __LINE__);
    for (uint32_t k = 0; k < P->shard_count; ++k)
        if (P->count[k] > shard_stride_tiles) return bad_arg(__func__, __LINE__);
    int e = bh_launch_tiles_unpack_rgbm(packed, out, out_bo, P->width, P->height, P->shard_count, shard_stride_tiles,
                                        P->tile_loc, format, rows_in_flight, reinterpret_cast<hipStream_t>(stream));
    if (e != 0) return hip_fail((hipError_t)e, "tiles unpack launch");
    return BH_OK;
}

int64_t bh_tile_bytes(uint32_t layout, uint32_t format) {
    if (format > BH_OUT_BGRA8_SRGB) return bad_arg(__func__, __LINE__);
    const int64_t bpp = format == BH_OUT_RGBA32F ? 16 : format == BH_OUT_RGBA16F ? 8 : 4;
    switch (layout) {
        case BH_LAYOUT_TILES: return 64 * bpp;
        case BH_LAYOUT_TILES_RGB: return 48 * bpp;
        case BH_LAYOUT_TILES_RGBM: return 48 * bpp + 8;
        case BH_LAYOUT_TILES_RGBM14: return format == BH_OUT_RGBA16F ? 344 : BH_ERR_UNSUPPORTED;
        default: return bad_arg(__func__, __LINE__);
    }
}

}  // extern "C"
