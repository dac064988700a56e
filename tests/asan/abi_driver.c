/* Host-side exercise of the C ABI for the AddressSanitizer build (make -C sat-bundleadjust_amd/csrc asan_lib): argument checks,
 * error strings and handle lifetime -- the paths that run without a GPU (in a container without one every call that needs the
 * device must come back with SATBA_E_HIP and a message, never crash).  tests/test_host_logic.py builds and runs it.
 * ("-fsanitize=address host build of the C-ABI shim".) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "satba.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) { fprintf(stderr, "abi_driver: %s failed (line %d): %s\n", #cond, __LINE__, satba_last_error()); return 1; } \
    } while (0)

/* a stand-alone entry point called with valid arguments: it succeeds with a GPU and names the HIP error without one */
#define CHECK_RUN(gpu, call)                                                                \
    do {                                                                                    \
        const int rc_ = (call);                                                             \
        if (gpu) CHECK(rc_ == SATBA_OK);                                                    \
        else CHECK(rc_ == SATBA_E_HIP && strlen(satba_last_error()) > 0);                   \
    } while (0)

/* a smooth, invertible RPC: the image coordinates are nearly linear in longitude, latitude and altitude */
static void rpc_table(double* t, double tilt) {
    memset(t, 0, sizeof(double) * SATBA_RPC_TABLE_LEN);
    t[1] = 1.0; t[2] = 0.1; t[3] = tilt;     /* col_num */
    t[20] = 1.0;                             /* col_den */
    t[41] = -0.1; t[42] = 1.0; t[43] = 0.05; /* row_num */
    t[60] = 1.0;                             /* row_den */
    const double ofs[10] = {10.0, 0.1, 45.0, 0.1, 100.0, 500.0, 5000.0, 5000.0, 5000.0, 5000.0};
    memcpy(t + 80, ofs, sizeof ofs);
}

/* cameras from RPCs and the fundamental matrices of their pairs */
static int check_cameras(int gpu) {
    double tab[2 * SATBA_RPC_TABLE_LEN], bad[SATBA_RPC_TABLE_LEN], P[12], mean_err[1], centers[3];
    rpc_table(tab, 0.05); rpc_table(tab + SATBA_RPC_TABLE_LEN, -0.08);
    memcpy(bad, tab, sizeof bad);
    bad[7] = strtod("nan", NULL);
    const double xyz[3] = {4449000.0, 784500.0, 4487400.0}, c0[2] = {0.0, 0.0};  /* near lon 10, lat 45 */
    CHECK(satba_rpc_affine_approx(-1, tab, xyz, c0, P, 0) == SATBA_E_ARG && satba_rpc_affine_approx(1, tab, xyz, c0, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_rpc_affine_approx(1, bad, xyz, c0, P, 0) == SATBA_E_NONFINITE && satba_rpc_affine_approx(0, tab, xyz, c0, P, 0) == SATBA_OK);
    CHECK_RUN(gpu, satba_rpc_affine_approx(1, tab, xyz, c0, P, 0));
    const double cr[2] = {0.0, 10000.0}, rr[2] = {0.0, 10000.0}, ar[2] = {0.0, 200.0}, flat[2] = {3.0, 3.0};
    CHECK(satba_rpc_perspective_approx(1, tab, cr, rr, ar, 1, 2, 2, NULL, P, NULL, NULL, 0) == SATBA_E_ARG && strstr(satba_last_error(), "at least 2"));
    CHECK(satba_rpc_perspective_approx(1, tab, cr, NULL, ar, 2, 2, 2, NULL, P, NULL, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_rpc_perspective_approx(1, tab, cr, rr, ar, 2, 2, 2, NULL, NULL, NULL, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_rpc_perspective_approx(1, tab, cr, rr, flat, 2, 2, 2, NULL, P, NULL, NULL, 0) == SATBA_E_NONFINITE);
    CHECK(satba_rpc_perspective_approx(1, tab, cr, rr, ar, 2, 2, 2, bad + 7, P, NULL, NULL, 0) == SATBA_E_NONFINITE);
    CHECK_RUN(gpu, satba_rpc_perspective_approx(1, tab, cr, rr, ar, 3, 3, 3, c0, P, mean_err, centers, 0));
    double X[8 * 3], x[8 * 2], X_out[8 * 3], x_out[8 * 2], alt_out[8];
    for (int i = 0; i < 8; ++i) {  /* the corners of a cube seen by a pinhole five units away */
        X[3 * i] = i & 1; X[3 * i + 1] = (i >> 1) & 1; X[3 * i + 2] = (i >> 2) & 1;
        x[2 * i] = X[3 * i] / (X[3 * i + 2] + 5.0); x[2 * i + 1] = X[3 * i + 1] / (X[3 * i + 2] + 5.0);
    }
    CHECK(satba_camera_resection(1, 5, X, x, P, NULL, 0) == SATBA_E_ARG && satba_camera_resection(1, 8, NULL, x, P, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_camera_resection(-1, 8, X, x, P, NULL, 0) == SATBA_E_ARG && satba_camera_resection(0, 8, X, x, P, NULL, 0) == SATBA_OK);
    CHECK_RUN(gpu, satba_camera_resection(1, 8, X, x, P, mean_err, 0));
    CHECK(satba_rpc_mesh(1, NULL, cr, rr, ar, 2, 2, 2, X_out, x_out, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_rpc_mesh(1, tab, cr, rr, ar, 2, 2, 2, NULL, x_out, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_rpc_mesh(1, tab, cr, rr, ar, 2, 2, 1 << 20, X_out, x_out, NULL, 0) == SATBA_E_ARG && strstr(satba_last_error(), "mesh larger"));
    CHECK_RUN(gpu, satba_rpc_mesh(1, tab, cr, rr, ar, 2, 2, 2, X_out, x_out, alt_out, 0));

    const int32_t pair[2] = {0, 1}, far[2] = {0, 2};
    const double roi[4] = {1000.0, 1000.0, 500.0, 500.0}, thin[4] = {1000.0, 1000.0, 0.0, 500.0};
    double F5[5], sv[4];
    uint8_t degenerate[1];
    CHECK(satba_rpc_fundamental(2, tab, 1, pair, roi, 2, NULL, NULL, NULL, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_rpc_fundamental(2, tab, 1, pair, roi, 1, F5, NULL, NULL, NULL, 0) == SATBA_E_ARG && strstr(satba_last_error(), "samples per axis"));
    CHECK(satba_rpc_fundamental(2, tab, 1, far, roi, 2, F5, NULL, NULL, NULL, 0) == SATBA_E_ARG && strstr(satba_last_error(), "outside"));
    CHECK(satba_rpc_fundamental(2, tab, 1, pair, thin, 2, F5, NULL, NULL, NULL, 0) == SATBA_E_ARG && strstr(satba_last_error(), "w > 0"));
    CHECK(satba_rpc_fundamental(1, bad, 0, pair, roi, 2, F5, NULL, NULL, NULL, 0) == SATBA_E_NONFINITE);
    CHECK(satba_rpc_fundamental(2, tab, 0, pair, roi, 2, F5, NULL, NULL, NULL, 0) == SATBA_OK);
    CHECK_RUN(gpu, satba_rpc_fundamental(2, tab, 1, pair, roi, 2, F5, sv, NULL, degenerate, 0));
    return 0;
}

/* ranking and selection of tracks: one track of two observations */
static int check_tracks(int gpu) {
    const int64_t ofs[2] = {0, 2}, late[2] = {1, 2}, back[3] = {0, 2, 1};
    const int32_t cam[2] = {0, 1}, swapped[2] = {1, 0}, beyond[2] = {0, 2}, pair[2] = {0, 1};
    const double scale[2] = {1.0, 2.0};
    int32_t length[2], A[4], tree_of[1], n_trees = -1;
    double ks[2], kc[2], weights[2];
    int64_t n_selected = -1, rank[1];
    uint8_t keep[2];
    CHECK(satba_track_keys(-1, ofs, scale, NULL, length, ks, kc, 0) == SATBA_E_ARG && satba_track_keys(1, NULL, scale, NULL, length, ks, kc, 0) == SATBA_E_ARG);
    CHECK(satba_track_keys(1, late, scale, NULL, length, ks, kc, 0) == SATBA_E_ARG && strstr(satba_last_error(), "offsets out of range"));
    CHECK(satba_track_keys(2, back, scale, NULL, length, ks, kc, 0) == SATBA_E_ARG && strstr(satba_last_error(), "pt_ofs must not decrease"));
    CHECK(satba_track_keys(1, ofs, NULL, NULL, length, ks, kc, 0) == SATBA_E_ARG && strstr(satba_last_error(), "null observations"));
    CHECK_RUN(gpu, satba_track_keys(1, ofs, scale, NULL, length, ks, kc, 0));
    CHECK(satba_track_connectivity(2, 1, ofs, cam, NULL, 0, NULL, 0) == SATBA_E_ARG && satba_track_connectivity(0, 1, ofs, cam, NULL, 0, A, 0) == SATBA_E_ARG);
    CHECK(satba_track_connectivity(2, 1, late, cam, NULL, 0, A, 0) == SATBA_E_ARG && strstr(satba_last_error(), "offsets out of range"));
    CHECK(satba_track_connectivity(2, 1, ofs, NULL, NULL, 0, A, 0) == SATBA_E_ARG && strstr(satba_last_error(), "null observations"));
    CHECK(satba_track_connectivity(2, 1, ofs, swapped, NULL, 0, A, 0) == SATBA_E_ARG && strstr(satba_last_error(), "ascend strictly"));
    CHECK(satba_track_connectivity(2, 1, ofs, beyond, NULL, 0, A, 0) == SATBA_E_ARG && strstr(satba_last_error(), "camera index 2"));
    CHECK(satba_track_connectivity(46341, 1, ofs, cam, NULL, 0, A, 0) == SATBA_E_ARG && strstr(satba_last_error(), "46 341"));
    CHECK_RUN(gpu, satba_track_connectivity(2, 1, ofs, cam, NULL, 0, A, 0));
    const int32_t prio[3] = {0, 1, 2}, twice[3] = {0, 0, -1}, odd[3] = {5, -1, -1};
    CHECK(satba_select_tracks(2, 1, ofs, cam, scale, NULL, -1, prio, tree_of, &n_selected, &n_trees, NULL, NULL, 0, NULL) == SATBA_E_ARG);
    CHECK(satba_select_tracks(2, 1, ofs, cam, scale, NULL, 1, NULL, tree_of, &n_selected, &n_trees, NULL, NULL, 0, NULL) == SATBA_E_ARG);
    CHECK(satba_select_tracks(2, 1, ofs, cam, scale, NULL, 1, twice, tree_of, &n_selected, &n_trees, NULL, NULL, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "twice"));
    CHECK(satba_select_tracks(2, 1, ofs, cam, scale, NULL, 1, odd, tree_of, &n_selected, &n_trees, NULL, NULL, 0, NULL) == SATBA_E_ARG);
    CHECK(satba_select_tracks(2, 2, back, cam, scale, NULL, 1, prio, tree_of, &n_selected, &n_trees, NULL, NULL, 0, NULL) == SATBA_E_ARG);
    CHECK(satba_select_tracks(2, 1, ofs, cam, NULL, NULL, 1, prio, tree_of, &n_selected, &n_trees, NULL, NULL, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "null observations"));
    float ms = -1.0f;
    CHECK_RUN(gpu, satba_select_tracks(2, 1, ofs, cam, scale, NULL, 1, prio, tree_of, &n_selected, &n_trees, weights, rank, 0, &ms));
    if (gpu) CHECK(n_selected == 1 && n_trees == 1 && tree_of[0] == 0 && rank[0] == 0);
    CHECK(satba_tracks_have_pair(2, 1, ofs, cam, -1, pair, keep, 0) == SATBA_E_ARG && satba_tracks_have_pair(2, 1, ofs, cam, 1, pair, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_tracks_have_pair(2, 1, ofs, cam, 1, NULL, keep, 0) == SATBA_E_ARG && satba_tracks_have_pair(2, 1, ofs, swapped, 1, pair, keep, 0) == SATBA_E_ARG);
    CHECK(satba_tracks_have_pair(2, 0, ofs, cam, 1, pair, keep, 0) == SATBA_OK);  /* no track: no device call */
    CHECK_RUN(gpu, satba_tracks_have_pair(2, 1, ofs, cam, 1, pair, keep, 0));
    if (gpu) CHECK(keep[0] == 1);
    return 0;
}

/* the three result handles: built, fetched and destroyed with a GPU; created and freed again on the failure path without one */
static int check_handles(int gpu) {
    float ms = -1.0f;
    {   /* feature tracks: two images of one keypoint each, joined by one match */
        const int64_t kp_ofs[3] = {0, 1, 2}, late[3] = {1, 1, 2}, back[3] = {0, 2, 1};
        const float kp[6] = {1.0f, 2.0f, 1.5f, 3.0f, 4.0f, 2.5f};
        const int32_t match[4] = {0, 0, 0, 1}, self[4] = {0, 0, 1, 1}, beyond[4] = {1, 0, 0, 1}, pair[2] = {0, 1};
        satba_ftracks* t = (satba_ftracks*)0x1;
        int64_t counts[5], pt_ofs[2];
        int32_t cam_ind[2], kp_id[2];
        double obs[4], scale[2];
        CHECK(satba_ftracks_build(2, kp_ofs, kp, 1, match, 1, pair, 0, NULL, counts, 0, NULL) == SATBA_E_ARG);
        CHECK(satba_ftracks_build(0, kp_ofs, kp, 1, match, 1, pair, 0, &t, counts, 0, NULL) == SATBA_E_ARG);
        CHECK(satba_ftracks_build(2, kp_ofs, kp, 1, NULL, 1, pair, 0, &t, counts, 0, NULL) == SATBA_E_ARG && t == NULL && strstr(satba_last_error(), "null matches"));
        CHECK(satba_ftracks_build(2, late, kp, 1, match, 1, pair, 0, &t, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "start at 0"));
        CHECK(satba_ftracks_build(2, back, kp, 1, match, 1, pair, 0, &t, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "must not decrease"));
        CHECK(satba_ftracks_build(2, kp_ofs, NULL, 1, match, 1, pair, 0, &t, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "null keypoints"));
        CHECK(satba_ftracks_build(2, kp_ofs, kp, 1, self, 1, pair, 0, &t, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "joins two"));
        CHECK(satba_ftracks_build(2, kp_ofs, kp, 1, beyond, 1, pair, 0, &t, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "outside its image"));
        CHECK(satba_ftracks_fetch(NULL, pt_ofs, cam_ind, kp_id, obs, scale) == SATBA_E_ARG);
        satba_ftracks_destroy(NULL);
        t = (satba_ftracks*)0x1;
        CHECK_RUN(gpu, satba_ftracks_build(2, kp_ofs, kp, 1, match, 1, pair, 0, &t, counts, 0, &ms));
        if (gpu) {
            CHECK(t != NULL && counts[0] == 1 && counts[1] == 2);
            CHECK(satba_ftracks_fetch(t, pt_ofs, cam_ind, kp_id, obs, scale) == SATBA_OK && pt_ofs[1] == 2 && cam_ind[1] == 1 && obs[2] == 3.0);
            CHECK(satba_ftracks_fetch(t, NULL, NULL, NULL, NULL, NULL) == SATBA_OK);
            satba_ftracks_destroy(t);
        } else {
            CHECK(t == NULL);
        }
    }
    {   /* matching: two images of one keypoint each, one pair */
        float f0[132] = {10.0f, 10.0f, 1.0f, 0.0f}, f1[132] = {11.0f, 10.0f, 1.0f, 0.0f};
        for (int k = 4; k < 132; ++k) { f0[k] = (float)(k % 7); f1[k] = (float)(k % 5); }
        const double u0[2] = {100.0, 200.0}, u1[2] = {101.0, 201.0};
        const float* feat[2] = {f0, f1};
        const double* utm[2] = {u0, u1};
        const float* no_feat[2] = {f0, NULL};
        const int64_t n_kp[2] = {1, 1}, neg[2] = {1, -1};
        const int32_t pair[2] = {0, 1}, self[2] = {1, 1}, far[2] = {0, 2};
        const double box[4] = {-1e9, 1e9, -1e9, 1e9}, hole[4] = {-1e9, strtod("nan", NULL), -1e9, 1e9}, F5[5] = {0.0, 1.0, 0.0, -1.0, strtod("inf", NULL)};
        satba_matches* m = (satba_matches*)0x1;
        int64_t counts[4], pair_ofs[2];
        int32_t kp_i[1], kp_j[1];
        CHECK(satba_match_pairs(2, n_kp, feat, utm, 1, pair, box, NULL, 0.6f, 0.0f, 1, NULL, counts, 0, NULL) == SATBA_E_ARG);
        CHECK(satba_match_pairs(2, n_kp, feat, utm, 1, NULL, box, NULL, 0.6f, 0.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && m == NULL);
        CHECK(satba_match_pairs(2, n_kp, feat, utm, 1, pair, box, NULL, 0.0f, 0.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "thr must"));
        CHECK(satba_match_pairs(2, n_kp, feat, utm, 1, pair, box, F5, 0.6f, 0.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "epi_thr"));
        CHECK(satba_match_pairs(2, n_kp, feat, utm, 1, pair, box, F5, 0.6f, 1.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "not finite"));
        CHECK(satba_match_pairs(2, neg, feat, utm, 1, pair, box, NULL, 0.6f, 0.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "keypoint count"));
        CHECK(satba_match_pairs(2, n_kp, feat, utm, 1, self, box, NULL, 0.6f, 0.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "with itself"));
        CHECK(satba_match_pairs(2, n_kp, feat, utm, 1, far, box, NULL, 0.6f, 0.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "outside"));
        CHECK(satba_match_pairs(2, n_kp, feat, utm, 1, pair, hole, NULL, 0.6f, 0.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "NaN"));
        CHECK(satba_match_pairs(2, n_kp, no_feat, utm, 1, pair, box, NULL, 0.6f, 0.0f, 1, &m, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "no arrays"));
        CHECK(satba_matches_fetch(NULL, pair_ofs, kp_i, kp_j) == SATBA_E_ARG);
        satba_matches_destroy(NULL);
        m = (satba_matches*)0x1;
        CHECK_RUN(gpu, satba_match_pairs(2, n_kp, feat, utm, 1, pair, box, NULL, 0.6f, 0.0f, 1, &m, counts, 0, &ms));
        if (gpu) {  /* a single finite candidate always passes the relative test */
            CHECK(m != NULL && counts[0] == 1 && counts[1] == 2);
            CHECK(satba_matches_fetch(m, pair_ofs, kp_i, kp_j) == SATBA_OK && pair_ofs[0] == 0 && pair_ofs[1] == 1 && kp_i[0] == 0 && kp_j[0] == 0);
            CHECK(satba_matches_fetch(m, NULL, NULL, NULL) == SATBA_OK);
            satba_matches_destroy(m);
        } else {
            CHECK(m == NULL);
        }
    }
    for (int keep_planes = 0; keep_planes < 2; ++keep_planes) {  /* detection: a 12 x 12 image, its planes dropped and kept */
        float image[12 * 12];
        for (int i = 0; i < 144; ++i) image[i] = (float)((i * 37) % 11) / 11.0f;
        satba_sift* s = (satba_sift*)0x1;
        int64_t counts[6];
        CHECK(satba_sift_detect(NULL, 12, 12, 12, 0.0133f, 8, 3, keep_planes, &s, counts, 0, NULL) == SATBA_E_ARG);
        CHECK(satba_sift_detect(image, 12, 12, 12, 0.0133f, 8, 3, keep_planes, NULL, counts, 0, NULL) == SATBA_E_ARG);
        CHECK(satba_sift_detect(image, 11, 12, 12, 0.0133f, 8, 3, keep_planes, &s, counts, 0, NULL) == SATBA_E_ARG && s == NULL);
        CHECK(satba_sift_detect(image, 12, 12, 11, 0.0133f, 8, 3, keep_planes, &s, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "row_stride"));
        CHECK(satba_sift_detect(image, 12, 12, 12, 0.0133f, 8, 0, keep_planes, &s, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "nb_scales"));
        CHECK(satba_sift_detect(image, 12, 12, 12, 0.0133f, 0, 3, keep_planes, &s, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "nb_octaves"));
        CHECK(satba_sift_detect(image, 12, 12, 12, -1.0f, 8, 3, keep_planes, &s, counts, 0, NULL) == SATBA_E_ARG && strstr(satba_last_error(), "thresh_dog"));
        CHECK(satba_sift_fetch(NULL, NULL) == SATBA_E_ARG && satba_sift_fetch_plane(NULL, 0, 0, NULL, NULL, NULL) == SATBA_E_ARG);
        satba_sift_destroy(NULL);
        s = (satba_sift*)0x1;
        CHECK_RUN(gpu, satba_sift_detect(image, 12, 12, 12, 0.0133f, 8, 3, keep_planes, &s, counts, 0, &ms));
        if (gpu) {
            CHECK(s != NULL && counts[0] >= 0 && counts[1] >= 1 && counts[5] == 0);
            float* rows = (float*)malloc(sizeof(float) * 132 * (size_t)(counts[0] + 1));
            CHECK(rows != NULL && satba_sift_fetch(s, rows) == SATBA_OK);
            free(rows);
            int32_t w = 0, h = 0;
            if (keep_planes) {
                CHECK(satba_sift_fetch_plane(s, 0, 0, NULL, &w, &h) == SATBA_OK && w == 24 && h == 24);
                CHECK(satba_sift_fetch_plane(s, (int32_t)counts[1], 0, NULL, &w, &h) == SATBA_E_ARG);
                float* plane = (float*)malloc(sizeof(float) * (size_t)w * (size_t)h);
                CHECK(plane != NULL && satba_sift_fetch_plane(s, 0, 5, plane, NULL, NULL) == SATBA_OK && plane[0] == plane[0]);
                free(plane);
            } else {
                CHECK(satba_sift_fetch_plane(s, 0, 0, NULL, &w, &h) == SATBA_E_STATE);
            }
            satba_sift_destroy(s);
        } else {
            CHECK(s == NULL);
        }
    }
    return 0;
}

int main(void) {
    satba_problem* p = (satba_problem*)0x1;
    CHECK(satba_version() >= 3);
    CHECK(satba_problem_create(NULL, &p) == SATBA_E_ARG);
    satba_problem_desc d;
    memset(&d, 0, sizeof d);
    d.cam_model = 7;
    CHECK(satba_problem_create(&d, &p) == SATBA_E_ARG && p == NULL && strstr(satba_last_error(), "cam_model"));
    d.cam_model = SATBA_AFFINE; d.cam_param_len = 9;
    CHECK(satba_problem_create(&d, &p) == SATBA_E_ARG && strstr(satba_last_error(), "cam_param_len"));
    d.cam_param_len = 8; d.n_params = 4;
    CHECK(satba_problem_create(&d, &p) == SATBA_E_ARG && strstr(satba_last_error(), "n_params"));
    d.n_params = 5; d.n_cam = 0;
    CHECK(satba_problem_create(&d, &p) == SATBA_E_ARG);
    d.n_cam = 2; d.n_pts = 3; d.n_obs = 4; d.world = 1;
    CHECK(satba_problem_create(&d, &p) == SATBA_E_ARG && strstr(satba_last_error(), "null input"));
    double cams[16] = {0}, obs[8] = {0}, w[4] = {1, 1, 1, 1};
    int32_t ci[4] = {0, 1, 0, 1}, pi[4] = {0, 0, 1, 1};
    d.cam_params = cams; d.cam_ind = ci; d.pts_ind = pi; d.pts2d = obs; d.weights = w;
    d.n_cam_fix = 5;
    CHECK(satba_problem_create(&d, &p) == SATBA_E_ARG && strstr(satba_last_error(), "n_cam_fix"));
    d.n_cam_fix = 1; d.world = 2; d.rank = 2;
    CHECK(satba_problem_create(&d, &p) == SATBA_E_ARG && strstr(satba_last_error(), "rank"));
    d.world = 1; d.rank = 0;
    const int rc = satba_problem_create(&d, &p);
    if (rc == SATBA_OK) {  /* a GPU is present: a few calls on a live handle, then the teardown */
        double x[2 * 5 + 3 * 3] = {0};
        CHECK(satba_set_x(p, x) == SATBA_OK);
        CHECK(satba_set_x(p, NULL) == SATBA_E_ARG);
        CHECK(satba_prepare(p, 1) == SATBA_E_STATE);
        double err[4], cost = -1.0;
        CHECK(satba_reprojection_errors(p, NULL, NULL) == SATBA_E_ARG);
        CHECK(satba_reprojection_errors(p, err, &cost) == SATBA_OK && cost >= 0.0);
        double err2[4] = {-1.0, -1.0, -1.0, -1.0};
        CHECK(satba_reprojection_errors_fetch(p, err2) == SATBA_E_STATE);  /* no _begin yet */
        CHECK(satba_reprojection_errors_begin(p) == SATBA_OK && satba_reprojection_errors_fetch(p, NULL) == SATBA_E_ARG);
        CHECK(satba_reprojection_errors_fetch(p, err2) == SATBA_OK && memcmp(err, err2, sizeof err) == 0);
        CHECK(satba_configure(p, 9, 1.0) == SATBA_E_ARG && satba_configure(p, 1, -1.0) == SATBA_E_ARG);
        double out[16];
        CHECK(satba_get_info(p, out, 4) == SATBA_E_ARG && satba_get_info(p, out, 16) == SATBA_OK);
        satba_problem_destroy(p);
    } else {
        CHECK(rc == SATBA_E_HIP && p == NULL && strlen(satba_last_error()) > 0);
    }
    /* entry points that take no handle */
    CHECK(satba_set_x(NULL, NULL) == SATBA_E_ARG && satba_linearize(NULL) == SATBA_E_ARG && satba_accept(NULL) == SATBA_E_ARG);
    CHECK(satba_header_len(NULL) == 0 && satba_exchange_len(NULL) == 0 && satba_layout_len(NULL, 0) == -1);
    CHECK(satba_lm_run(NULL, 1, 0, 0.0, NULL, 0) == SATBA_E_ARG && satba_lm_state(NULL, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_reprojection_errors(NULL, NULL, NULL) == SATBA_E_ARG);
    CHECK(satba_reprojection_errors_begin(NULL) == SATBA_E_ARG && satba_reprojection_errors_fetch(NULL, NULL) == SATBA_E_ARG);
    CHECK(satba_rpc_fit(-1, 0, NULL, NULL, 1e-3, 1e-2, 20, NULL, NULL, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_rpc_refit(1, NULL, NULL, NULL, NULL, NULL, 10, 1e-3, 1e-2, 20, NULL, NULL, NULL, NULL, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_rpc_localization(NULL, 3, NULL, NULL, NULL, NULL, NULL, 0) == SATBA_E_ARG);
    CHECK(satba_triangulate_pairwise(SATBA_RPC, NULL, NULL, 1, NULL, NULL, NULL, NULL, 0, NULL) == SATBA_E_ARG);
    CHECK(satba_init_pts3d(SATBA_AFFINE, 2, 1, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, 1, NULL) == SATBA_E_ARG);
    {   /* the scalar side of the loop: argument checks, then the host compilation on the stalled bracket, a rank-one model and no radius */
        double in[18] = {-1, 0, 1, 1e-20, 0, 1, 1, 2, 4, -1, -2, 8, 2, 0, 1, 1, 1, 0}, out[18];
        CHECK(satba_lm_scalars(2, 1, in, out) == SATBA_E_ARG && satba_lm_scalars(0, -1, in, out) == SATBA_E_ARG);
        CHECK(satba_lm_scalars(0, 1, NULL, out) == SATBA_E_ARG && satba_lm_scalars(1, 1, in, NULL) == SATBA_E_ARG);
        CHECK(satba_lm_scalars(0, 0, NULL, NULL) == SATBA_OK && satba_lm_scalars(1, 0, NULL, NULL) == SATBA_OK);
        CHECK(satba_lm_scalars(0, 3, in, out) == SATBA_OK);
        CHECK(out[0] == -1.0 && out[1] == 0.0 && out[2] == 0.0);
        CHECK(out[6] == out[6] && out[7] == out[7] && out[6] * out[6] + out[7] * out[7] <= 64.0 * (1.0 + 1e-15));
        CHECK(out[12] == 0.0 && out[13] == 0.0 && out[14] == 0.0);
    }
    /* the stand-alone stages in front of the solver: argument checks, then one small valid call each */
    if (check_cameras(rc == SATBA_OK) || check_tracks(rc == SATBA_OK) || check_handles(rc == SATBA_OK)) return 1;
    satba_problem_destroy(NULL);
    printf("abi_driver ok\n");
    return 0;
}
