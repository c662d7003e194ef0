// check_resize_index.hip -- a stand-alone HOST check of the index logic of csrc/resize.hip, over the kernels' own
// __host__ __device__ text: for every axis pair it compares rz_reach_lo / rz_reach_hi with a brute-force scan of the tap ranges,
// checks that the ranges are monotone, that an area window stays inside the axis and that the dense matrix is zero outside a pixel's
// reach; for every shape it checks that each tile's staged block fits the host's plan, forward and backward.  No GPU is used.
//   hipcc -O1 --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Wno-unused-function \
//         -I single-image-super-resolution_amd/csrc tools/check_resize_index.hip -o /tmp/check_resize_index && /tmp/check_resize_index
#include "../single-image-super-resolution_amd/csrc/resize.hip"
#include <cstdio>
#include <vector>
static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)
static void axis(int n_in, int n_out) {
    for (int mode = 0; mode < 3; ++mode) {
        // dense matrix
        std::vector<double> R((size_t)n_out * n_in, 0.0);
        std::vector<int> lo(n_out), hi(n_out);
        for (int o = 0; o < n_out; ++o) {
            RzTap t = rz_tap(mode, n_in, n_out, o);
            lo[o] = rz_idx_lo(mode, n_in, n_out, o); hi[o] = rz_idx_hi(mode, n_in, n_out, o);
            if (o) CHECK(lo[o] >= lo[o-1] && hi[o] >= hi[o-1], "monotone %d %d %d %d", mode, n_in, n_out, o);
            if (mode == 0) CHECK(t.first >= 0 && t.first + t.count <= n_in, "area window %d %d %d", n_in, n_out, o);
            for (int k = 0; k < t.count; ++k) R[(size_t)o * n_in + rz_clamp(t.first + k, 0, n_in - 1)] += t.w[mode == 0 ? 0 : k];
        }
        for (int i = 0; i < n_in; ++i) {
            int blo = n_out, bhi = -1;
            for (int o = 0; o < n_out; ++o) if (lo[o] <= i && i <= hi[o]) { if (blo == n_out) blo = o; bhi = o; }
            const int rlo = rz_reach_lo(mode, n_in, n_out, i), rhi = rz_reach_hi(mode, n_in, n_out, i);
            if (blo <= bhi) CHECK(rlo == blo && rhi == bhi, "reach mode %d %d->%d i %d: %d..%d vs %d..%d", mode, n_in, n_out, i, rlo, rhi, blo, bhi);
            else CHECK(rlo > rhi, "empty reach mode %d %d->%d i %d: %d..%d", mode, n_in, n_out, i, rlo, rhi);
            // outside the reach the dense matrix is zero
            for (int o = 0; o < n_out; ++o) if (o < rlo || o > rhi) CHECK(R[(size_t)o * n_in + i] == 0.0, "outside reach");
        }
    }
}
static void plans(int H, int W, int h, int w) {
    const RzPlans& pl = rz_plans(H, W, h, w);
    printf("%dx%d -> %dx%d  fwd tile %dx%d stage %dx%d %lld B   bwd tile %dx%d stage %dx%d %lld B\n", H, W, h, w, pl.fwd.TH, pl.fwd.TW, pl.fwd.SH, pl.fwd.SW,
           (long long)(4 * pl.fwd.words), pl.bwd.TH, pl.bwd.TW, pl.bwd.SH, pl.bwd.SW, (long long)(4 * pl.bwd.words));
    for (int mode = 0; mode < 3; ++mode) {
        for (int o0 = 0; o0 < h; o0 += pl.fwd.TH) { int o1 = std::min(o0 + pl.fwd.TH, h) - 1; CHECK(rz_idx_hi(mode, H, h, o1) - rz_idx_lo(mode, H, h, o0) + 1 <= pl.fwd.SH, "fwd SH"); }
        for (int o0 = 0; o0 < w; o0 += pl.fwd.TW) { int o1 = std::min(o0 + pl.fwd.TW, w) - 1; CHECK(rz_idx_hi(mode, W, w, o1) - rz_idx_lo(mode, W, w, o0) + 1 <= pl.fwd.SW, "fwd SW"); }
        for (int i0 = 0; i0 < H; i0 += pl.bwd.TH) { int i1 = std::min(i0 + pl.bwd.TH, H) - 1; CHECK(rz_reach_hi(mode, H, h, i1) - rz_reach_lo(mode, H, h, i0) + 1 <= pl.bwd.SH, "bwd SH");
            for (int i = i0; i <= i1; ++i) CHECK(rz_reach_lo(mode, H, h, i) >= rz_reach_lo(mode, H, h, i0) && rz_reach_hi(mode, H, h, i) <= rz_reach_hi(mode, H, h, i1), "bwd nest"); }
        for (int i0 = 0; i0 < W; i0 += pl.bwd.TW) { int i1 = std::min(i0 + pl.bwd.TW, W) - 1; CHECK(rz_reach_hi(mode, W, w, i1) - rz_reach_lo(mode, W, w, i0) + 1 <= pl.bwd.SW, "bwd SW"); }
    }
}
int main() {
    const int sh[][4] = {{1,1,1,1},{7,5,3,4},{5,7,11,13},{33,35,8,9},{40,70,37,67},{16,16,8,8},{8,8,16,16},{3,50,9,2},{1,9,4,1},{192,192,136,136},{192,192,96,96},{96,96,192,192},
                         {24,20,17,13},{17,13,12,10},{256,256,16,16},{16,16,256,256},{12,12,400,400},{2000,2000,5,5},{24,24,24,24},{17,13,17,13},{130,20,9,300},{70,130,9,17}};
    for (auto& s : sh) { axis(s[0], s[2]); axis(s[1], s[3]); plans(s[0], s[1], s[2], s[3]); }
    for (int a = 1; a <= 40; ++a) for (int b = 1; b <= 40; ++b) axis(a, b);
    printf("bad = %d\n", bad);
    return bad != 0;
}
int sisr_device_index() { return 0; }          // misc.hip's, for the launch helpers that this program never calls
