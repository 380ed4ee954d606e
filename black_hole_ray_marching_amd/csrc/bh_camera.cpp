// bh_camera.cpp — the host math of the ABI that needs no device: the scene's default uniforms, the glam-style
// camera, its controller and uniform (the kernels' inputs, bit for bit the reference's), and the synthetic sky.
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "bh_host.hpp"

namespace {

// ---- glam 0.24 Vec3 subset (scalar f32, left-to-right association as glam writes it) ----------
struct V3 { float x, y, z; };
V3 v_add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 v_sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 v_mul(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
float v_dot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
V3 v_cross(V3 a, V3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
V3 v_normalize(V3 a) { return v_mul(a, 1.0f / std::sqrt(v_dot(a, a))); }  // self * length_recip()
V3 v_neg(V3 a) { return {-a.x, -a.y, -a.z}; }

// glam 0.24 Quat (f32): from_axis_angle and mul_vec3 (the SSE2 path evaluates the same formula with
// the same operand order: dot = (x + y) + z, no FMA)
struct Q4 { float x, y, z, w; };
Q4 q_from_axis_angle(V3 axis, float angle) {
    const float h = angle * 0.5f;
    const float s = std::sin(h), c = std::cos(h);  // f32::sin_cos
    const V3 v = v_mul(axis, s);
    return {v.x, v.y, v.z, c};
}
V3 q_mul_vec3(Q4 q, V3 rhs) {
    const float w = q.w;
    const V3 b{q.x, q.y, q.z};
    const float b2 = v_dot(b, b);
    return v_add(v_add(v_mul(rhs, w * w - b2), v_mul(b, v_dot(rhs, b) * 2.0f)), v_mul(v_cross(b, rhs), w * 2.0f));
}
float axis_norm(uint8_t neg, uint8_t pos) { return (neg == pos) ? 0.0f : (pos ? 1.0f : -1.0f); }

uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t hash3(uint64_t seed, int64_t a, int64_t b, int64_t c) {
    uint64_t s = seed ^ ((uint64_t)a * 0x9E3779B185EBCA87ull) ^ ((uint64_t)b * 0xC2B2AE3D27D4EB4Full) ^
                 ((uint64_t)c * 0x165667B19E3779F9ull);
    return splitmix64(s);
}
float unit(uint64_t h) { return (float)(h >> 40) * (1.0f / 16777216.0f); }

// periodic-in-x lattice value noise, smoothstep interpolation
float value_noise(uint64_t seed, int oct, float x, float y, int period_x) {
    float fx = std::floor(x), fy = std::floor(y);
    int ix = (int)fx, iy = (int)fy;
    float tx = x - fx, ty = y - fy;
    tx = tx * tx * (3.0f - 2.0f * tx);
    ty = ty * ty * (3.0f - 2.0f * ty);
    auto L = [&](int cx, int cy) {
        int wx = ((cx % period_x) + period_x) % period_x;
        return unit(hash3(seed, oct, wx, cy));
    };
    float a = L(ix, iy), b = L(ix + 1, iy), c = L(ix, iy + 1), d = L(ix + 1, iy + 1);
    return (a + (b - a) * tx) + ((c + (d - c) * tx) - (a + (b - a) * tx)) * ty;
}

uint8_t encode8(float lin) {
    if (!(lin > 0.0f)) return 0;
    if (lin >= 1.0f) return 255;
    double v = lin, s = v <= 0.0031308 ? 12.92 * v : 1.055 * std::pow(v, 1.0 / 2.4) - 0.055;
    return (uint8_t)std::floor(s * 255.0 + 0.5);
}

}  // namespace

extern "C" {

// Scene::new defaults, src/scene.rs:89-137 (RS 1.0, max dt 0.5, bg 0.5, blackout PodBool::r#false()
// whose inner is 1 (src/podbool.rs:24-26), max dist 250, distortion 1.0); 24 B padded to 32.
int bh_uniforms_default(bh_uniforms* out) {
    if (!out) return bad_arg(__func__, __LINE__);
    std::memset(out, 0, sizeof(*out));
    out->rs = 1.0f;
    out->delta_time_mult = 0.5f;
    out->bg_brightness = 0.5f;
    out->blackout_eh = 1u;
    out->max_dist = 250.0f;
    out->distortion_power = 1.0f;
    return BH_OK;
}

// src/scene.rs:68-76
int bh_camera_default(uint32_t width, uint32_t height, bh_camera* out) {
    if (!out || width == 0 || height == 0) return bad_arg(__func__, __LINE__);
    const float PI = 3.14159265358979323846f;  // std::f32::consts::PI
    *out = bh_camera{{0.0f, 0.0f, -20.0f}, {0.0f, 0.0f, 1.0f}, {0.0f, 1.0f, 0.0f},
                     (float)width / (float)height, PI * 0.5f, 0.1f, 100.0f};
    return BH_OK;
}

int bh_controller_update(const bh_controller* k, bh_camera* cam, float dt, int do_pan, int* moved) {
    if (!k || !cam) return bad_arg(__func__, __LINE__);
    V3 pos{cam->pos[0], cam->pos[1], cam->pos[2]};
    V3 dir{cam->dir[0], cam->dir[1], cam->dir[2]};
    V3 up{cam->up[0], cam->up[1], cam->up[2]};
    auto right = [&] { return v_cross(up, dir); };  // Camera::right = up x dir (camera.rs:32)
    const float xn = axis_norm(k->left, k->right), zn = axis_norm(k->backward, k->forward);
    const float yn = axis_norm(k->down, k->up);
    const float xm = dt * k->speed * xn, zm = dt * k->speed * zn, ym = dt * k->speed * yn;
    pos = v_add(pos, v_mul(right(), xm));
    pos = v_add(pos, v_mul(dir, zm));
    pos = v_add(pos, v_mul(up, ym));
    const float en = axis_norm(k->exp_towards_origin, k->exp_away_origin);
    pos = v_mul(pos, std::exp(-dt * en));
    const float xpn = axis_norm(k->pan_left, k->pan_right), ypn = axis_norm(k->pan_up, k->pan_down);
    const float xp = dt * k->pan_speed * xpn, yp = dt * k->pan_speed * ypn;
    auto rotate = [&](V3 axis, float angle) {
        const Q4 q = q_from_axis_angle(axis, angle);
        dir = q_mul_vec3(q, dir);
        up = q_mul_vec3(q, up);
    };
    rotate(V3{0.0f, 1.0f, 0.0f}, xp);
    rotate(right(), yp);
    float mx = 0.0f, my = 0.0f;  // cursor_movement (camera.rs:268-278)
    if (k->has_prev_cursor && k->has_curr_cursor) {
        mx = k->curr_cursor[0] - k->prev_cursor[0];
        my = k->curr_cursor[1] - k->prev_cursor[1];
    }
    const float ps = dt * k->pan_speed;
    if (k->mouse_pressed && do_pan) {
        rotate(V3{0.0f, 1.0f, 0.0f}, ps * mx);
        rotate(right(), ps * my);
    }
    cam->pos[0] = pos.x; cam->pos[1] = pos.y; cam->pos[2] = pos.z;
    cam->dir[0] = dir.x; cam->dir[1] = dir.y; cam->dir[2] = dir.z;
    cam->up[0] = up.x; cam->up[1] = up.y; cam->up[2] = up.z;
    if (moved) *moved = (xn != 0.0f) | (yn != 0.0f) | (zn != 0.0f) | (xpn != 0.0f) | (ypn != 0.0f);
    return BH_OK;
}

int bh_camera_look_at(const float pos[3], const float target[3], uint32_t width, uint32_t height,
                      bh_camera* out) {
    if (!pos || !target) return bad_arg(__func__, __LINE__);
    int st = bh_camera_default(width, height, out);
    if (st != BH_OK) return st;
    V3 p{pos[0], pos[1], pos[2]}, t{target[0], target[1], target[2]};
    V3 d = v_normalize(v_sub(t, p));
    std::memcpy(out->pos, pos, 3 * sizeof(float));
    out->dir[0] = d.x; out->dir[1] = d.y; out->dir[2] = d.z;
    return BH_OK;
}

// CameraUniform::new (src/uniforms.rs:108-122) + ::update (:123-133) ->
// Camera::pos_to_world_space_screen_triangle (src/camera.rs:89-112):
//   corner_i = rot_matrix * ( -(tx * cx_i), -(-ty) * cy_i ... ) — concretely
//   dir_camera = -vec3(tx*cx, -ty*cy, 1)  (camera.rs:70-74),
//   rot_matrix = look_at_rh(pos, pos + dir, up).inverse()  (camera.rs:56-58),
//   world = rot_matrix.transform_vector3(dir_camera)  (camera.rs:76).
// The view matrix is a rigid transform, so its inverse's rotation block is the transpose
// (columns s, u, -f).  glam's general f32 Mat4::inverse may differ from the transpose in the last
// ulp; the corners are kernel INPUTS, so this host step is outside kernel parity.
int bh_camera_uniform_update(const bh_camera* cam, bh_camera_uniform* out) {
    if (!cam || !out) return bad_arg(__func__, __LINE__);
    std::memset(out, 0, sizeof(*out));
    static const float st[3][2] = {{3.0f, 1.0f}, {-1.0f, 1.0f}, {-1.0f, -3.0f}};
    for (int i = 0; i < 3; ++i) { out->screen_tri[i][0] = st[i][0]; out->screen_tri[i][1] = st[i][1]; }
    V3 pos{cam->pos[0], cam->pos[1], cam->pos[2]};
    V3 dir{cam->dir[0], cam->dir[1], cam->dir[2]};
    V3 up{cam->up[0], cam->up[1], cam->up[2]};
    // look_at_rh(eye, center, up) = look_to_rh(eye, center - eye, up)
    V3 f = v_normalize(v_sub(v_add(pos, dir), pos));
    V3 s = v_normalize(v_cross(f, up));
    V3 u = v_cross(s, f);
    V3 col0 = s, col1 = u, col2 = v_neg(f);
    // tan_fov_half (camera.rs:60-63)
    float tfy = std::tan(cam->fovy / 2.0f);
    float tfx = tfy * cam->aspect;
    for (int i = 0; i < 3; ++i) {
        float cx = st[i][0], cy = st[i][1];
        V3 dc = v_neg(V3{tfx * cx, -tfy * cy, 1.0f});
        // transform_vector3: res = x_axis*x; res = y_axis*y + res; res = z_axis*z + res
        V3 res = v_mul(col0, dc.x);
        res = v_add(v_mul(col1, dc.y), res);
        res = v_add(v_mul(col2, dc.z), res);
        out->world_tri[i][0] = res.x; out->world_tri[i][1] = res.y; out->world_tri[i][2] = res.z;
        out->world_tri[i][3] = 0.0f;
    }
    out->pos[0] = pos.x; out->pos[1] = pos.y; out->pos[2] = pos.z;
    return BH_OK;
}

// The ray map of bh_render's own projection: pixel_ray's interpolated vector d (bh_march_step.hpp) before its
// normalisation, by the same fp32 operations in the same order -- the IEEE divisions by 2W and 2H (what the kernel's
// division core returns), l1 = (1 - l0) - l2, (l0 c0 + l1 c1) + l2 c2.  This unit is built without contraction.
int bh_ray_map_pinhole_host(const bh_camera_uniform* cam, uint32_t width, uint32_t height, float* out) {
    if (!cam || !out || width == 0 || height == 0 || width > 65536u || height > 65536u) return bad_arg(__func__, __LINE__);
    static const float st[3][2] = {{3.0f, 1.0f}, {-1.0f, 1.0f}, {-1.0f, -3.0f}};
    for (int i = 0; i < 3; ++i)
        if (cam->screen_tri[i][0] != st[i][0] || cam->screen_tri[i][1] != st[i][1]) {
            bh_set_last_error("bh_ray_map_pinhole_host: non-default screen triangle");
            return BH_ERR_UNSUPPORTED;
        }
    const float w2 = 2.0f * (float)width, h2 = 2.0f * (float)height;
    for (uint32_t y = 0; y < height; ++y) {
        const float l2 = ((float)y + 0.5f) / h2;
        for (uint32_t x = 0; x < width; ++x) {
            const float l0 = ((float)x + 0.5f) / w2;
            const float l1 = (1.0f - l0) - l2;
            float* d = out + ((size_t)y * width + x) * 3u;
            for (int k = 0; k < 3; ++k)
                d[k] = (l0 * cam->world_tri[0][k] + l1 * cam->world_tri[1][k]) + l2 * cam->world_tri[2][k];
        }
    }
    return BH_OK;
}

static void sky_rows(uint8_t* out, uint32_t w, uint32_t h, uint64_t seed, uint32_t y0, uint32_t y1) {
    const int base = 6;  // nebula lattice cells around the equator at octave 0
    for (uint32_t y = y0; y < y1; ++y) {
        for (uint32_t x = 0; x < w; ++x) {
            float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)h;
            float n1 = 0.0f, n2 = 0.0f, amp = 0.5f;
            for (int o = 0; o < 5; ++o) {
                int per = base << o;
                n1 += amp * value_noise(seed, o, u * per, v * (per / 2), per);
                n2 += amp * value_noise(seed ^ 0xA5A5A5A5ull, o, u * per, v * (per / 2), per);
                amp *= 0.5f;
            }
            float neb = std::fmax(0.0f, n1 - 0.45f) * 1.6f;
            float r = 0.012f + 0.55f * neb * neb + 0.10f * n2 * neb;
            float g = 0.010f + 0.22f * neb * n2;
            float b = 0.030f + 0.65f * neb * (1.0f - 0.5f * n2);
            uint64_t hs = hash3(seed ^ 0x5354415253ull, 99, x, y);  // "STARS"
            if ((hs & 0xFFFu) < 6u) {                                // ~0.15 % of texels
                float mag = unit(hs);
                float temp = unit(hs * 0x2545F4914F6CDD1Dull);
                float L = 0.25f + 0.75f * mag * mag;
                r += L * (0.8f + 0.2f * temp);
                g += L * 0.85f;
                b += L * (1.0f - 0.3f * temp);
            }
            uint8_t* p = out + ((size_t)y * w + x) * 4u;
            p[0] = encode8(r); p[1] = encode8(g); p[2] = encode8(b); p[3] = 255;
        }
    }
}

// Rows are independent, so the result does not depend on the thread count.
int bh_synthetic_sky(uint8_t* out, uint32_t w, uint32_t h, uint64_t seed) {
    if (!out || w == 0 || h == 0) return bad_arg(__func__, __LINE__);
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : (nt > 16 ? 16 : nt);
    if (nt > h) nt = h;
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t) {
        uint32_t y0 = (uint32_t)((uint64_t)h * t / nt), y1 = (uint32_t)((uint64_t)h * (t + 1) / nt);
        pool.emplace_back(sky_rows, out, w, h, seed, y0, y1);
    }
    for (auto& th : pool) th.join();
    return BH_OK;
}

}  // extern "C"
