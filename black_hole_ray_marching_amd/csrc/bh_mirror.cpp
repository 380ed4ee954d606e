// bh_mirror.cpp — CPU mirrors of device code, the references of the tests: each runs the very functions its
// kernel runs per lane (bh_ss.hpp, bh_lens.hpp, bh_refine.hpp) in loops over the frame.  Nothing here renders.
#include <cmath>
#include <cstring>
#include <new>

#include "bh_host.hpp"
#include "bh_lens.hpp"
#include "bh_refine.hpp"
#include "bh_shutter.hpp"
#include "bh_ss.hpp"

extern "C" {

// The posed ray-map kernels' turn of a map's vector on the host (march_slot's POSE form, bh_march_tile.hpp):
// (mx r + my u) + mz f per component, one statement per operation -- this unit is built without contraction.
int bh_ray_pose_apply_host(const bh_ray_pose* pose, const float* dirs, uint32_t width, uint32_t height, float* out) {
    if (!pose || !dirs || !out || width == 0 || height == 0 || width > 65536u || height > 65536u) return bad_arg(__func__, __LINE__);
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i) {
        const float mx = dirs[3u * i], my = dirs[3u * i + 1u], mz = dirs[3u * i + 2u];
        for (int k = 0; k < 3; ++k) {
            const float a = mx * pose->r[k];
            const float b = my * pose->u[k];
            const float ab = a + b;
            const float c = mz * pose->f[k];
            out[3u * i + (size_t)k] = ab + c;
        }
    }
    return BH_OK;
}

// The origin-map kernels' ray origin on the host (org_frame, bh_march_tile.hpp): pos + ((ox r + oy u) + oz f) per
// component, one statement per operation.  Each pixel's three inputs are read before its outputs are written, so
// `out` may be `origins`.
int bh_ray_origins_apply_host(const bh_ray_pose* pose, const float* origins, uint32_t width, uint32_t height, float* out) {
    if (!pose || !origins || !out || width == 0 || height == 0 || width > 65536u || height > 65536u) return bad_arg(__func__, __LINE__);
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i) {
        const float ox = origins[3u * i], oy = origins[3u * i + 1u], oz = origins[3u * i + 2u];
        for (int k = 0; k < 3; ++k) {
            const float a = ox * pose->r[k];
            const float b = oy * pose->u[k];
            const float ab = a + b;
            const float c = oz * pose->f[k];
            const float w = ab + c;
            out[3u * i + (size_t)k] = pose->pos[k] + w;
        }
    }
    return BH_OK;
}

// The supersampled march kernel's epilogue on the host: the functions of bh_ss.hpp that each lane of a wave
// runs (ss_resolve_store, bh_march_resolve.hpp), run here wave by wave over 64-entry arrays -- one 8x8 tile of the
// virtual frame per wave, invalid lanes 0, every lane taking each butterfly level together.
int bh_ss_resolve_host(const float* samples, uint32_t width, uint32_t height, uint32_t ss, float* out) {
    const uint32_t lk = bh::ss::log2_k(ss);
    if (!samples || !out || lk > 3u) return bad_arg(__func__, __LINE__);
    if (!frame_shape_ok(width, height, ss)) return bad_arg(__func__, __LINE__);
    const uint32_t vw = width * ss, vh = height * ss;
    const uint32_t tiles_x = (vw + 7u) / 8u, tiles_y = (vh + 7u) / 8u;
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) {
            float v[3][64], nv[64];
            bool valid[64];
            for (uint32_t lane = 0; lane < 64u; ++lane) {
                const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
                valid[lane] = px < vw && py < vh;
                for (int ch = 0; ch < 3; ++ch)
                    v[ch][lane] = valid[lane] ? samples[((size_t)py * vw + px) * 4u + (size_t)ch] : 0.0f;
            }
            for (int ch = 0; ch < 3; ++ch) {
                float* cur = v[ch];
                for (uint32_t i = 0; i < bh::ss::levels(lk); ++i) {
                    const uint32_t mask = bh::ss::level_mask(i, lk);
                    for (uint32_t lane = 0; lane < 64u; ++lane)
                        nv[lane] = bh::ss::level_add(cur[lane], mask, [&](uint32_t m) { return cur[lane ^ m]; });
                    std::memcpy(cur, nv, sizeof nv);
                }
            }
            for (uint32_t lane = 0; lane < 64u; ++lane) {
                if (!(valid[lane] && bh::ss::writer(lane, lk))) continue;
                const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
                float* o = out + (size_t)bh::ss::out_index(px, py, lk, width) * 4u;
                for (int ch = 0; ch < 3; ++ch) o[ch] = v[ch][lane] * bh::ss::scale(lk);
                o[3] = 1.0f;
            }
        }
    return BH_OK;
}

// The shutter kernel's resolve on the host: bh_shutter.hpp's mapping and tree, workgroup by workgroup.  Workgroup
// g's wave w takes the dispatch slot the kernel's wave takes (wave_slot), decoded as march_slot decodes it (order
// index slot / n_cameras, camera slot % n_cameras; the order here is the identity: any order visits every tile);
// its 64 lanes hold the camera's samples of that tile of the virtual frame, through bh_ss.hpp's butterfly and
// scale when ss > 1; then the writer lanes sum the n waves' values in tree order, scale and store.
int bh_shutter_resolve_host(const float* samples, uint32_t n_frames, uint32_t n_sub, uint32_t width, uint32_t height,
                            uint32_t ss, float* out) {
    const uint32_t lk = bh::ss::log2_k(ss), ln = bh::shutter::log2_n(n_sub);
    if (!samples || !out || lk > 3u || ln > bh::shutter::MAX_LOG2) return bad_arg(__func__, __LINE__);
    if (n_frames == 0u || (uint64_t)n_frames * n_sub > BH_MAX_FRAMES) return bad_arg(__func__, __LINE__);
    if (!frame_shape_ok(width, height, ss)) return bad_arg(__func__, __LINE__);
    const uint32_t vw = width * ss, vh = height * ss, n_cams = n_frames << ln;
    const uint32_t tiles_x = (vw + 7u) / 8u, tiles_y = (vh + 7u) / 8u, n_tiles = tiles_x * tiles_y;
    const size_t vpx = (size_t)vw * vh, opx = (size_t)width * height;
    std::vector<uint8_t> visits, stores;
    std::vector<float> wave;  // [wave][channel][lane]
    try {
        visits.assign((size_t)n_cams * n_tiles, 0u);
        stores.assign((size_t)n_frames * opx, 0u);
        wave.resize((size_t)n_sub * 3u * 64u);
    } catch (const std::bad_alloc&) {
        return BH_ERR_OUT_OF_MEMORY;
    }
    bool outside = false;
    for (uint32_t g = 0; g < n_tiles * n_frames; ++g) {
        const uint32_t f = bh::shutter::group_frame(g, n_frames);
        uint32_t tile = 0;
        for (uint32_t w = 0; w < n_sub; ++w) {
            const uint32_t slot = bh::shutter::wave_slot(g, w, n_frames, ln);
            const uint32_t j = slot / n_cams, cam = slot - j * n_cams;
            if (j >= n_tiles || cam >= n_cams || (w != 0u && j != tile)) { outside = true; continue; }
            tile = j;
            if (visits[(size_t)cam * n_tiles + j] != 255u) ++visits[(size_t)cam * n_tiles + j];
            const uint32_t ty = j / tiles_x, tx = j - ty * tiles_x;
            const float* S = samples + (size_t)cam * vpx * 4u;
            float nv[64];
            for (int ch = 0; ch < 3; ++ch) {
                float* cur = &wave[((size_t)w * 3u + (size_t)ch) * 64u];
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
                    cur[lane] = px < vw && py < vh ? S[((size_t)py * vw + px) * 4u + (size_t)ch] : 0.0f;
                }
                if (lk == 0u) continue;
                for (uint32_t i = 0; i < bh::ss::levels(lk); ++i) {
                    const uint32_t mask = bh::ss::level_mask(i, lk);
                    for (uint32_t lane = 0; lane < 64u; ++lane)
                        nv[lane] = bh::ss::level_add(cur[lane], mask, [&](uint32_t m) { return cur[lane ^ m]; });
                    std::memcpy(cur, nv, sizeof nv);
                }
                for (uint32_t lane = 0; lane < 64u; ++lane) cur[lane] = cur[lane] * bh::ss::scale(lk);
            }
        }
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
            if (!(px < vw && py < vh && bh::ss::writer(lane, lk))) continue;
            const size_t idx = bh::ss::out_index(px, py, lk, width);
            if (idx >= opx) { outside = true; continue; }
            if (stores[(size_t)f * opx + idx] != 255u) ++stores[(size_t)f * opx + idx];
            float* o = out + ((size_t)f * opx + idx) * 4u;
            for (int ch = 0; ch < 3; ++ch) {
                const float s = bh::shutter::tree_sum(ln, [&](uint32_t t) { return wave[((size_t)t * 3u + (size_t)ch) * 64u + lane]; });
                o[ch] = s * bh::shutter::scale(ln);
            }
            o[3] = 1.0f;
        }
    }
    bool once = !outside;
    for (uint8_t v : visits) once = once && v == 1u;
    for (uint8_t v : stores) once = once && v == 1u;
    if (!once) {
        bh_set_last_error("bh_shutter_resolve_host: a (frame, tile, camera) not visited exactly once, or a store outside the frame");
        return BH_ERR_INTERNAL;
    }
    return BH_OK;
}

// The shade kernels' per-pixel function (bh_lens.hpp, shade_pixel) in a loop over the output frame, for the
// plain shade's lens or the filtered one's.
extern "C++" template <int K, class L>
static void lens_shade_rows(const L& lens, uint32_t width, uint32_t height, float* out_col, float* out_bo) {
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const bh::lens::Acc p = out_bo ? bh::lens::shade_pixel<K, true>(lens, x, y) : bh::lens::shade_pixel<K, false>(lens, x, y);
            const bh::lens::Rgb col = p.col, bo = p.bo;
            const size_t o = ((size_t)y * width + x) * 4u;
            out_col[o] = col.r; out_col[o + 1] = col.g; out_col[o + 2] = col.b; out_col[o + 3] = 1.0f;
            if (out_bo) { out_bo[o] = bo.r; out_bo[o + 1] = bo.g; out_bo[o + 2] = bo.b; out_bo[o + 3] = 1.0f; }
        }
}

// A sky as the device holds it: the decode table, and the packed little-endian words the kernels read (the
// caller's bytes may be unaligned).  False: out of memory.
struct HostSky {
    float lut[256];
    std::vector<uint32_t> texels;
    bh::lens::SkyView view;
};
static bool host_sky(const uint8_t* sky, uint32_t sky_w, uint32_t sky_h, HostSky* k) {
    srgb_lut(k->lut);
    try {
        k->texels.resize((size_t)sky_w * sky_h);
    } catch (const std::bad_alloc&) {
        return false;
    }
    std::memcpy(k->texels.data(), sky, k->texels.size() * 4u);
    k->view = {k->texels.data(), sky_w, sky_h};
    return true;
}

int bh_lens_shade_host(const bh_lens_px* lens, uint32_t width, uint32_t height, uint32_t ss, const uint8_t* sky,
                       uint32_t sky_w, uint32_t sky_h, float* out_col, float* out_bo) {
    if (!lens || !sky || !out_col || bh::ss::log2_k(ss) > 3u || !frame_shape_ok(width, height, ss)) return bad_arg(__func__, __LINE__);
    if (sky_w == 0 || sky_h == 0 || sky_w > 32768u || sky_h > 32768u) return bad_arg(__func__, __LINE__);
    HostSky k;
    if (!host_sky(sky, sky_w, sky_h, &k)) return BH_ERR_OUT_OF_MEMORY;
    const bh::lens::PlainLens l{lens, width, k.view, k.lut};
    switch (ss) {
        case 1u: lens_shade_rows<1>(l, width, height, out_col, out_bo); break;
        case 2u: lens_shade_rows<2>(l, width, height, out_col, out_bo); break;
        case 4u: lens_shade_rows<4>(l, width, height, out_col, out_bo); break;
        default: lens_shade_rows<8>(l, width, height, out_col, out_bo); break;
    }
    return BH_OK;
}

// What both disc mirrors refuse, and their loop over either lens (bh_lens.hpp, DiscLens and BeamLens).
static bool disc_host_ok(const bh_lens_px* lens, const float* hits, uint32_t width, uint32_t height, uint32_t ss,
                         const uint8_t* sky, uint32_t sky_w, uint32_t sky_h, const uint8_t* disc, uint32_t n_phi,
                         uint32_t n_r, uint32_t scene_flags, float spin, float gain, const float* out_col) {
    if (!lens || !hits || !sky || !disc || !out_col || bh::ss::log2_k(ss) > 3u || !frame_shape_ok(width, height, ss)) return false;
    if (sky_w == 0 || sky_h == 0 || sky_w > 32768u || sky_h > 32768u) return false;
    if (n_phi == 0 || n_r == 0 || n_phi > 32768u || n_r > 32768u || (scene_flags & ~BH_SCENE_DEFAULT)) return false;
    return std::isfinite(spin) && std::isfinite(gain) && gain >= 0.0f;
}
extern "C++" template <class Lens>
static void lens_shade_any(const Lens& l, uint32_t width, uint32_t height, uint32_t ss, float* out_col, float* out_bo) {
    switch (ss) {
        case 1u: lens_shade_rows<1>(l, width, height, out_col, out_bo); break;
        case 2u: lens_shade_rows<2>(l, width, height, out_col, out_bo); break;
        case 4u: lens_shade_rows<4>(l, width, height, out_col, out_bo); break;
        default: lens_shade_rows<8>(l, width, height, out_col, out_bo); break;
    }
}

// bh_shade_lens_disc on the host: the disc shade's lens (bh_lens.hpp, DiscLens) through the same loop.
int bh_lens_shade_disc_host(const bh_lens_px* lens, const float* hits, uint32_t width, uint32_t height, uint32_t ss,
                            const uint8_t* sky, uint32_t sky_w, uint32_t sky_h, const uint8_t* disc, uint32_t n_phi,
                            uint32_t n_r, float rs, uint32_t scene_flags, float spin, float gain, float* out_col,
                            float* out_bo) {
    if (!disc_host_ok(lens, hits, width, height, ss, sky, sky_w, sky_h, disc, n_phi, n_r, scene_flags, spin, gain, out_col))
        return bad_arg(__func__, __LINE__);
    HostSky k, dk;  // the disc's texels travel as a sky's do
    if (!host_sky(sky, sky_w, sky_h, &k) || !host_sky(disc, n_phi, n_r, &dk)) return BH_ERR_OUT_OF_MEMORY;
    const bh::lens::DiscLens l{lens, hits, width, k.view, {dk.texels.data(), n_phi, n_r, rs, scene_flags, spin, gain}, k.lut};
    lens_shade_any(l, width, height, ss, out_col, out_bo);
    return BH_OK;
}

// bh_shade_lens_disc_beamed on the host: BeamLens through the same loop.
int bh_lens_shade_disc_beamed_host(const bh_lens_px* lens, const float* hits, uint32_t width, uint32_t height, uint32_t ss,
                                   const uint8_t* sky, uint32_t sky_w, uint32_t sky_h, const uint8_t* disc, uint32_t n_phi,
                                   uint32_t n_r, float rs, uint32_t scene_flags, float spin, float gain, float* out_col,
                                   float* out_bo, const float* arrivals, float beam, int32_t sense, float distortion_power) {
    if (!disc_host_ok(lens, hits, width, height, ss, sky, sky_w, sky_h, disc, n_phi, n_r, scene_flags, spin, gain, out_col))
        return bad_arg(__func__, __LINE__);
    if (!arrivals || (sense != 1 && sense != -1) || !(beam >= 0.0f && beam <= 1.0f) || !std::isfinite(distortion_power))
        return bad_arg(__func__, __LINE__);
    HostSky k, dk;
    if (!host_sky(sky, sky_w, sky_h, &k) || !host_sky(disc, n_phi, n_r, &dk)) return BH_ERR_OUT_OF_MEMORY;
    const bh::lens::BeamLens l{lens, hits, arrivals, width, k.view, {dk.texels.data(), n_phi, n_r, rs, scene_flags, spin, gain},
                               {beam, (float)sense, distortion_power}, k.lut};
    lens_shade_any(l, width, height, ss, out_col, out_bo);
    return BH_OK;
}

// The chain kernels' per-texel functions (bh_lens.hpp, mip_down0 and mip_down) level after level: levels 1 ..
// `upto` of the sky, back to back at mip_offsets' places.
static void build_chain(const bh::lens::SkyView& s, const float* lut, uint32_t upto, const uint32_t* off, bh::lens::Half4* chain) {
    for (uint32_t l = 1; l <= upto; ++l) {
        const uint32_t sw = bh::lens::mip_side(s.w, l - 1u), sh = bh::lens::mip_side(s.h, l - 1u);
        const uint32_t w = bh::lens::mip_side(s.w, l), h = bh::lens::mip_side(s.h, l);
        for (uint32_t j = 0; j < h; ++j)
            for (uint32_t i = 0; i < w; ++i)
                bh::lens::store_half4(chain + off[l] + j * w + i, l == 1u ? bh::lens::mip_down0(s, lut, i, j)
                                                                         : bh::lens::mip_down(chain + off[l - 1u], sw, sh, i, j));
    }
}

int bh_sky_mips_host(const uint8_t* sky, uint32_t sky_w, uint32_t sky_h, uint32_t level, uint16_t* out_halves) {
    if (!sky || !out_halves || sky_w == 0 || sky_h == 0 || sky_w > 32768u || sky_h > 32768u) return bad_arg(__func__, __LINE__);
    if (level < 1u || level >= bh::lens::mip_levels(sky_w, sky_h)) return bad_arg(__func__, __LINE__);
    uint32_t off[bh::lens::MIP_MAX_LEVELS];
    bh::lens::mip_offsets(sky_w, sky_h, off);
    const size_t n_out = (size_t)bh::lens::mip_side(sky_w, level) * bh::lens::mip_side(sky_h, level);
    HostSky k;
    std::vector<bh::lens::Half4> chain;
    try {
        chain.resize(off[level] + n_out);
    } catch (const std::bad_alloc&) {
        return BH_ERR_OUT_OF_MEMORY;
    }
    if (!host_sky(sky, sky_w, sky_h, &k)) return BH_ERR_OUT_OF_MEMORY;
    build_chain(k.view, k.lut, level, off, chain.data());
    std::memcpy(out_halves, chain.data() + off[level], n_out * sizeof(bh::lens::Half4));
    return BH_OK;
}

int bh_lens_shade_mip_host(const bh_lens_px* lens, uint32_t width, uint32_t height, uint32_t ss, const uint8_t* sky,
                           uint32_t sky_w, uint32_t sky_h, float* out_col, float* out_bo) {
    if (!lens || !sky || !out_col || bh::ss::log2_k(ss) > 3u || !frame_shape_ok(width, height, ss)) return bad_arg(__func__, __LINE__);
    if (sky_w == 0 || sky_h == 0 || sky_w > 32768u || sky_h > 32768u) return bad_arg(__func__, __LINE__);
    if (ss == 8u) {
        bh_set_last_error("bh_lens_shade_mip_host: ss = 8 is not built (bh_shade_lens_mip).");
        return BH_ERR_UNSUPPORTED;
    }
    uint32_t off[bh::lens::MIP_MAX_LEVELS];
    const size_t n_chain = bh::lens::mip_offsets(sky_w, sky_h, off);
    const uint32_t n_levels = bh::lens::mip_levels(sky_w, sky_h);
    HostSky k;
    std::vector<bh::lens::Half4> chain;
    try {
        chain.resize(n_chain);
    } catch (const std::bad_alloc&) {
        return BH_ERR_OUT_OF_MEMORY;
    }
    if (!host_sky(sky, sky_w, sky_h, &k)) return BH_ERR_OUT_OF_MEMORY;
    build_chain(k.view, k.lut, n_levels - 1u, off, chain.data());
    const bh::lens::MipLens l{lens, width, height, {k.view, chain.data(), off, n_levels}, k.lut};
    switch (ss) {
        case 1u: lens_shade_rows<1>(l, width, height, out_col, out_bo); break;
        case 2u: lens_shade_rows<2>(l, width, height, out_col, out_bo); break;
        default: lens_shade_rows<4>(l, width, height, out_col, out_bo); break;
    }
    return BH_OK;
}

// The detect kernel's decision on the host: bh_refine.hpp's lane function, tile by tile and lane by lane.
int bh_refine_mask_host(const void* col, const void* blackout, uint32_t width, uint32_t height, uint32_t format,
                        float threshold, uint8_t* tile_mask) {
    if (!col || !tile_mask || width == 0 || height == 0 || width > 32768u || height > 32768u) return bad_arg(__func__, __LINE__);
    if (format > BH_OUT_BGRA8_SRGB || !(threshold >= 0.0f) || std::isinf(threshold)) return bad_arg(__func__, __LINE__);
    const uint32_t tiles_x = bh::refine::tiles_of(width), tiles_y = bh::refine::tiles_of(height);
    const float thr = bh::refine::threshold(format, threshold);
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) {
            bool any = false;  // the wave's ballot
            for (uint32_t lane = 0; lane < 64u; ++lane)
                any |= bh::refine::lane_edge(format, col, blackout, width, height, tx, ty, lane, thr);
            tile_mask[(size_t)ty * tiles_x + tx] = any ? 1u : 0u;
        }
    return BH_OK;
}

// The work-list march's stores on the host: the list a detect pass would leave for this mask (both ends used),
// every work item mapped by bh_refine.hpp's item functions, every lane of its wave through bh_ss.hpp's writer
// and output index.  An index outside the frame is counted nowhere and fails the call.
int bh_refine_cover_host(uint32_t width, uint32_t height, uint32_t ss, const uint8_t* tile_mask, uint8_t* pixel_writes) {
    const uint32_t lk = bh::ss::log2_k(ss);
    if (!tile_mask || !pixel_writes || lk < 1u || lk > 3u) return bad_arg(__func__, __LINE__);
    if (!frame_shape_ok(width, height, ss)) return bad_arg(__func__, __LINE__);
    const uint32_t tiles_x = bh::refine::tiles_of(width), tiles_y = bh::refine::tiles_of(height);
    const uint32_t vw = width * ss, vh = height * ss;
    const uint32_t vtiles_x = bh::refine::tiles_of(vw), vtiles_y = bh::refine::tiles_of(vh);
    const size_t n_px = (size_t)width * height;
    std::memset(pixel_writes, 0, n_px);
    // filled from both ends as the detect kernel fills it (every third refined tile to the front)
    const uint32_t capacity = tiles_x * tiles_y;
    std::vector<uint32_t> list(capacity, 0xFFFFFFFFu);
    uint32_t n_front = 0, n_back = 0;
    for (uint32_t t = 0, n = 0; t < capacity; ++t)
        if (tile_mask[t]) list[n++ % 3u == 0u ? n_front++ : capacity - 1u - n_back++] = t;
    if (((uint64_t)(n_front + n_back) << (2u * lk)) > 0xFFFF0000ull) return bad_arg(__func__, __LINE__);
    const uint32_t total = (n_front + n_back) << (2u * lk);
    bool outside = false;
    for (uint32_t item = 0; item < total; ++item) {
        uint32_t vtx, vty;
        const uint32_t slot = bh::refine::entry_slot(bh::refine::item_entry(item, lk), n_front, capacity);
        if (!bh::refine::item_tile(list[slot], bh::refine::item_sub(item, lk), lk, tiles_x,
                                   tiles_y, vtiles_x, vtiles_y, &vtx, &vty))
            continue;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint32_t px = bh::refine::lane_x(vtx, lane), py = bh::refine::lane_y(vty, lane);
            if (!(px < vw && py < vh && bh::ss::writer(lane, lk))) continue;
            const size_t idx = bh::ss::out_index(px, py, lk, width);
            if (idx >= n_px) { outside = true; continue; }
            if (pixel_writes[idx] != 255u) ++pixel_writes[idx];
        }
    }
    if (outside) {
        bh_set_last_error("bh_refine_cover_host: a store index outside the frame");
        return BH_ERR_INTERNAL;
    }
    return BH_OK;
}

}  // extern "C"
