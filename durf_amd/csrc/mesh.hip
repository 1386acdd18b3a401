// The iso-surface of a density lattice as an indexed triangle mesh (include/durf_mesh.h; libdurf_mesh.so): marching tetrahedra
// on the Kuhn subdivision with welded vertices.  Classify and count per lattice point (k_mesh_classify), one workgroup's
// exclusive scan of the block sums (k_scan_block_sums), offsets (k_mesh_offsets) -- the three plain passes of scan.h --,
// then emit (k_mesh_emit) and the attribute gather (k_mesh_gather).  Streaming kernels, one thread per lattice point with
// adjacent lanes along k, plain fp32 in the order the header states; no atomics, nothing synchronises or copies to the host.
#include "workspace.h"
#include "scan.h"
#include "lattice.h"
#include "../../include/durf_mesh.h"

#define MESH_B DURF_MESH_BLOCK
#define MESH_WAVES (MESH_B / DURF_WAVE)

// ---- the sixteen cases, built from the header's rule ------------------------------------------------------------------------
// A cell corner is the code c = 4 di + 2 dj + dk; the edge from corner a to corner b (a's bits a subset of b's) is edge
// e = b - a - 1 of the lattice point at corner a.  A tetrahedron's edges are the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) of
// its local corners.
struct MeshTables {
    unsigned char corner[6][4];        // cell-corner code of local corner l of tetrahedron t
    unsigned char eown[6][6];          // cell-corner code of the lattice point that owns tetrahedron edge E
    unsigned char eedge[6][6];         // and which of its seven edges that is
    unsigned char ntri[16];            // triangles of case (bit l: local corner l is in)
    unsigned char tri[6][16][6];       // tetrahedron edges of up to two triangles, wound for a right-handed frame
    bool ok;                           // no triangle of the construction is degenerate
};

constexpr int mesh_te(int a, int b) { return a == 0 ? b - 1 : a == 1 ? b + 1 : 5; }      // (a < b) -> 0 .. 5

constexpr MeshTables mesh_make_tables() {
    MeshTables T{};
    T.ok = true;
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const int pair[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
    for (int t = 0; t < 6; t++) {
        T.corner[t][0] = 0;
        T.corner[t][1] = (unsigned char)(4 >> perm[t][0]);
        T.corner[t][2] = (unsigned char)(T.corner[t][1] | (4 >> perm[t][1]));
        T.corner[t][3] = 7;
        for (int E = 0; E < 6; E++) {
            const int a = T.corner[t][pair[E][0]], b = T.corner[t][pair[E][1]];
            T.eown[t][E] = (unsigned char)a;
            T.eedge[t][E] = (unsigned char)(b - a - 1);
        }
        for (int cs = 0; cs < 16; cs++) {
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int l = 0; l < 4; l++) {
                if (cs >> l & 1) in[ni++] = l; else out[no++] = l;
            }
            int tr[6] = {}, nt = 0;
            if (ni == 1 || no == 1) {
                const int a = ni == 1 ? in[0] : out[0];
                int k = 0;
                for (int l = 0; l < 4; l++)
                    if (l != a) tr[k++] = l < a ? mesh_te(l, a) : mesh_te(a, l);
                nt = 1;
            } else if (ni == 2) {
                const int a = in[0], b = in[1], c = out[0], d = out[1];
                auto e = [](int x, int y) { return x < y ? mesh_te(x, y) : mesh_te(y, x); };
                const int ac = e(a, c), ad = e(a, d), bd = e(b, d), bc = e(b, c);
                tr[0] = ac; tr[1] = ad; tr[2] = bd; tr[3] = ac; tr[4] = bd; tr[5] = bc;
                nt = 2;
            }
            if (t == 0) T.ntri[cs] = (unsigned char)nt;
            // the winding: edge midpoints (twice them, integers) in index space, whose frame is right-handed; the right-hand
            // normal must point along mean(O) - mean(I) (here scaled by |I| |O|)
            int dir[3] = {};
            for (int x = 0; x < 3; x++) {
                int so = 0, si = 0;
                for (int l = 0; l < no; l++) so += T.corner[t][out[l]] >> (2 - x) & 1;
                for (int l = 0; l < ni; l++) si += T.corner[t][in[l]] >> (2 - x) & 1;
                dir[x] = ni * so - no * si;
            }
            for (int r = 0; r < nt; r++) {
                int M[3][3] = {};
                for (int v = 0; v < 3; v++)
                    for (int x = 0; x < 3; x++) {
                        const int E = tr[3 * r + v];
                        M[v][x] = (T.corner[t][pair[E][0]] >> (2 - x) & 1) + (T.corner[t][pair[E][1]] >> (2 - x) & 1);
                    }
                int u[3] = {}, w[3] = {};
                for (int x = 0; x < 3; x++) { u[x] = M[1][x] - M[0][x]; w[x] = M[2][x] - M[0][x]; }
                const int s = (u[1] * w[2] - u[2] * w[1]) * dir[0] + (u[2] * w[0] - u[0] * w[2]) * dir[1] +
                              (u[0] * w[1] - u[1] * w[0]) * dir[2];
                if (s == 0) T.ok = false;
                if (s < 0) { const int x = tr[3 * r + 1]; tr[3 * r + 1] = tr[3 * r + 2]; tr[3 * r + 2] = x; }
            }
            for (int q = 0; q < 6; q++) T.tri[t][cs][q] = (unsigned char)tr[q];
        }
    }
    return T;
}

constexpr bool mesh_parity_rule(const MeshTables& T) {
    // permutations 0, 3, 4 are even, 1, 2, 5 odd: the winding depends on the case and the parity alone
    for (int cs = 0; cs < 16; cs++)
        for (int q = 0; q < 6; q++) {
            if (T.tri[3][cs][q] != T.tri[0][cs][q] || T.tri[4][cs][q] != T.tri[0][cs][q]) return false;
            if (T.tri[2][cs][q] != T.tri[1][cs][q] || T.tri[5][cs][q] != T.tri[1][cs][q]) return false;
        }
    return true;
}

constexpr MeshTables MESH_TABLES = mesh_make_tables();
static_assert(MESH_TABLES.ok, "no case has a degenerate triangle");
static_assert(mesh_parity_rule(MESH_TABLES), "the winding depends on the case and the parity of the permutation");
static_assert(MESH_TABLES.ntri[0] == 0 && MESH_TABLES.ntri[15] == 0 && MESH_TABLES.ntri[1] == 1 && MESH_TABLES.ntri[3] == 2 &&
              MESH_TABLES.ntri[14] == 1, "0, 1 or 2 triangles");
static_assert(MESH_TABLES.corner[3][1] == 2 && MESH_TABLES.corner[3][2] == 3, "permutation (1,2,0): +j, then +k");
__constant__ MeshTables c_mesh = MESH_TABLES;

// ---- the lattice (lattice.h) ----------------------------------------------------------------------------------------------------
// the eight corners of the cell at (i, j, k): bit c of *exist (the corner is inside the lattice), *usable, *in
__device__ __forceinline__ void mesh_corners(const LatticeDims D, const float* __restrict__ density, const uint8_t* __restrict__ valid,
                                             float iso, int g, int i, int j, int k, unsigned* exist, unsigned* usable, unsigned* in) {
    unsigned X = 0, U = 0, N = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        int di, dj, dk;
        lattice_corner(c, di, dj, dk);
        if (i + di < D.nu && j + dj < D.nv && k + dk < D.nw) {
            X |= 1u << c;
            float d;
            if (lattice_usable(density, valid, g + lattice_index(D, di, dj, dk), &d)) {
                U |= 1u << c;
                if (d >= iso) N |= 1u << c;
            }
        }
    }
    *exist = X; *usable = U; *in = N;
}

// pass 1: per lattice point the seven activity bits and the counts of its vertices (into voff) and of its cell's triangles
// (into toff); per workgroup the two sums
__global__ void __launch_bounds__(MESH_B)
k_mesh_classify(const LatticeDims D, const float* __restrict__ density, const uint8_t* __restrict__ valid, float iso,
                int32_t* __restrict__ voff, int32_t* __restrict__ toff, uint8_t* __restrict__ mask, int32_t* __restrict__ sums_v,
                int32_t* __restrict__ sums_t) {
    __shared__ int s_v[MESH_WAVES], s_t[MESH_WAVES];
    const int t = threadIdx.x, g = blockIdx.x * MESH_B + t;
    int cv = 0, ct = 0;
    if (g < D.n) {
        int i, j, k;
        lattice_ijk(D, g, i, j, k);
        unsigned X, U, N;
        mesh_corners(D, density, valid, iso, g, i, j, k, &X, &U, &N);
        unsigned m = 0;
        if (U & 1u) {
#pragma unroll
            for (int e = 0; e < 7; e++)
                if ((U >> (e + 1) & 1u) && ((N >> (e + 1) ^ N) & 1u)) m |= 1u << e;
        }
        cv = __popc(m);
        if (X >> 7 & 1u) {
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const unsigned c1 = c_mesh.corner[q][1], c2 = c_mesh.corner[q][2];
                if ((U & 1u) && (U >> c1 & 1u) && (U >> c2 & 1u) && (U >> 7 & 1u))
                    ct += c_mesh.ntri[(N & 1u) | (N >> c1 & 1u) << 1 | (N >> c2 & 1u) << 2 | (N >> 7 & 1u) << 3];
            }
        }
        mask[g] = (uint8_t)m;
        voff[g] = cv;
        toff[g] = ct;
    }
    scan_wave_to_lds(cv, s_v);
    scan_wave_to_lds(ct, s_t);
    __syncthreads();
    if (t == 0) {
        sums_v[blockIdx.x] = scan_block_sum<MESH_WAVES>(s_v);
        sums_t[blockIdx.x] = scan_block_sum<MESH_WAVES>(s_t);
    }
}

// pass 2: k_scan_block_sums<int32_t, 2> (scan.h) on the two rows sums_v, sums_t = sums_v + nb + 1; the totals go to counts

// pass 3: the per-point counts in voff and toff become the exclusive prefix sums in g order
__global__ void __launch_bounds__(MESH_B)
k_mesh_offsets(int n, int32_t* __restrict__ voff, int32_t* __restrict__ toff, const int32_t* __restrict__ sums_v,
               const int32_t* __restrict__ sums_t) {
    __shared__ int s_v[MESH_WAVES], s_t[MESH_WAVES];
    const int g = blockIdx.x * MESH_B + threadIdx.x;
    const int cv = g < n ? voff[g] : 0, ct = g < n ? toff[g] : 0;
    const int iv = scan_wave_to_lds(cv, s_v), it = scan_wave_to_lds(ct, s_t);
    __syncthreads();
    if (g >= n) return;
    voff[g] = scan_before_wave<MESH_WAVES>(sums_v[blockIdx.x], s_v) + (iv - cv);
    toff[g] = scan_before_wave<MESH_WAVES>(sums_t[blockIdx.x], s_t) + (it - ct);
}

// ---- emit -------------------------------------------------------------------------------------------------------------------
struct MeshNormals { float A[9]; };    // the inverse transpose of [du dv dw]

// the index-space gradient at lattice point (i, j, k), index g, whose density d0 is usable
__device__ __forceinline__ void mesh_gradient(const LatticeDims D, const float* __restrict__ density, const uint8_t* __restrict__ valid,
                                              int g, int i, int j, int k, float d0, float* gr) {
    const int at[3] = {i, j, k}, dim[3] = {D.nu, D.nv, D.nw}, stride[3] = {D.nv * D.nw, D.nw, 1};
#pragma unroll
    for (int x = 0; x < 3; x++) {
        float dp = 0.0f, dm = 0.0f;
        const bool up = at[x] + 1 < dim[x] && lattice_usable(density, valid, g + stride[x], &dp);
        const bool um = at[x] > 0 && lattice_usable(density, valid, g - stride[x], &dm);
        gr[x] = up && um ? 0.5f * (dp - dm) : up ? dp - d0 : um ? d0 - dm : 0.0f;
    }
}

__global__ void __launch_bounds__(MESH_B)
k_mesh_emit(const LatticeDims D, const float* __restrict__ density, const uint8_t* __restrict__ valid, float iso, const LatticeFrame F,
            const MeshNormals M, int flip, const int32_t* __restrict__ voff, const int32_t* __restrict__ toff, const uint8_t* __restrict__ mask,
            int max_vertices, int max_triangles, float* __restrict__ vertices, float* __restrict__ normals,
            int32_t* __restrict__ vertex_edge, float* __restrict__ vertex_t, int32_t* __restrict__ triangles) {
    const int g = blockIdx.x * MESH_B + threadIdx.x;
    if (g >= D.n) return;
    int i, j, k;
    lattice_ijk(D, g, i, j, k);
    // the vertices on this point's active edges
    const unsigned m = mask[g];
    if (m) {
        int id = voff[g];
        const float da = density[g];
        float gra[3];
        if (normals) mesh_gradient(D, density, valid, g, i, j, k, da, gra);
        for (int e = 0; e < 7; e++) {
            if (!(m >> e & 1u)) continue;
            const int v = id++;
            if ((unsigned)v >= (unsigned)max_vertices) continue;
            int di, dj, dk;
            lattice_edge(e, di, dj, dk);
            // an active edge exists: its far end is inside the lattice (bounds: mask comes from k_mesh_classify's own test,
            // and a stale workspace is caught here)
            if (i + di >= D.nu || j + dj >= D.nv || k + dk >= D.nw) continue;
            const int gb = g + lattice_index(D, di, dj, dk);
            const float db = density[gb];
            float t = (iso - da) / (db - da);
            t = fminf(fmaxf(t, 0.0f), 1.0f);
            lattice_point(F, (float)i + t * (float)di, (float)j + t * (float)dj, (float)k + t * (float)dk, vertices + (size_t)v * 3);
            if (vertex_edge) { vertex_edge[(size_t)v * 2] = g; vertex_edge[(size_t)v * 2 + 1] = e; }
            if (vertex_t) vertex_t[v] = t;
            if (normals) {
                float grb[3], gr[3], mm[3];
                mesh_gradient(D, density, valid, gb, i + di, j + dj, k + dk, db, grb);
#pragma unroll
                for (int x = 0; x < 3; x++) gr[x] = gra[x] + t * (grb[x] - gra[x]);
#pragma unroll
                for (int c = 0; c < 3; c++) mm[c] = (M.A[c * 3] * gr[0] + M.A[c * 3 + 1] * gr[1]) + M.A[c * 3 + 2] * gr[2];
                const float len = sqrtf((mm[0] * mm[0] + mm[1] * mm[1]) + mm[2] * mm[2]);
                float nn[3];
                bool fine = true;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    nn[c] = -mm[c] / len;
                    fine = fine && fabsf(nn[c]) <= 3.0e38f;                 // (false for NaN and the infinities)
                }
                fine = fine && (nn[0] != 0.0f || nn[1] != 0.0f || nn[2] != 0.0f);
#pragma unroll
                for (int c = 0; c < 3; c++) normals[(size_t)v * 3 + c] = fine ? nn[c] : 0.0f;
            }
        }
    }
    // the triangles of the cell at this point
    if (i >= D.nu - 1 || j >= D.nv - 1 || k >= D.nw - 1) return;
    unsigned X, U, N;
    mesh_corners(D, density, valid, iso, g, i, j, k, &X, &U, &N);
    int tid = toff[g];
    for (int q = 0; q < 6; q++) {
        const unsigned c1 = c_mesh.corner[q][1], c2 = c_mesh.corner[q][2];
        if (!((U & 1u) && (U >> c1 & 1u) && (U >> c2 & 1u) && (U >> 7 & 1u))) continue;
        const unsigned cs = (N & 1u) | (N >> c1 & 1u) << 1 | (N >> c2 & 1u) << 2 | (N >> 7 & 1u) << 3;
        const int nt = c_mesh.ntri[cs];
        for (int r2 = 0; r2 < nt; r2++) {
            const int at = tid++;
            if ((unsigned)at >= (unsigned)max_triangles) continue;
            int ids[3];
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const int E = c_mesh.tri[q][cs][3 * r2 + v];
                const int c = c_mesh.eown[q][E], e = c_mesh.eedge[q][E];
                const int gg = g + lattice_corner_offset(D, c);                                // a corner of an existing cell
                ids[v] = voff[gg] + __popc(mask[gg] & ((1u << e) - 1u));
            }
            int32_t* row = triangles + (size_t)at * 3;
            row[0] = ids[0];
            row[1] = flip ? ids[2] : ids[1];
            row[2] = flip ? ids[1] : ids[2];
        }
    }
}

// ---- lattice attributes at the vertices --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_B)
k_mesh_gather(const LatticeDims D, const int32_t* __restrict__ counts, int max_vertices, const int32_t* __restrict__ vertex_edge,
              const float* __restrict__ vertex_t, int C, const float* __restrict__ attr_f, float* __restrict__ out_f,
              const int32_t* __restrict__ attr_i, const float* __restrict__ density, const uint8_t* __restrict__ valid, float iso,
              int32_t* __restrict__ out_i) {
    const int v = blockIdx.x * MESH_B + threadIdx.x;
    if (v >= max_vertices || v >= counts[0]) return;
    const int g = vertex_edge[(size_t)v * 2], e = vertex_edge[(size_t)v * 2 + 1];
    if (g < 0 || g >= D.n || e < 0 || e > 6) return;
    int i, j, k, di, dj, dk;
    lattice_ijk(D, g, i, j, k);
    lattice_edge(e, di, dj, dk);
    if (i + di >= D.nu || j + dj >= D.nv || k + dk >= D.nw) return;
    const int gb = g + lattice_index(D, di, dj, dk);
    if (attr_f) {
        const float t = vertex_t[v];
        for (int c = 0; c < C; c++) {
            const float a = attr_f[(size_t)g * C + c], b = attr_f[(size_t)gb * C + c];
            out_f[(size_t)v * C + c] = a + t * (b - a);
        }
    }
    if (attr_i) {
        float da;
        const bool a_in = lattice_usable(density, valid, g, &da) && da >= iso;
        out_i[v] = attr_i[a_in ? g : gb];
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
namespace {

struct MeshWs {
    int32_t *voff, *toff;
    uint8_t* mask;
    int32_t *sums_v, *sums_t;
    int nb;
    size_t total;
};

MeshWs carve_mesh(void* base, int n) {
    durf::Carver c{(char*)base, 0};
    MeshWs w{};
    w.nb = (int)durf_cdiv((size_t)n, MESH_B);
    w.voff = (int32_t*)c.take((size_t)n * 4);
    w.toff = (int32_t*)c.take((size_t)n * 4);
    w.mask = (uint8_t*)c.take((size_t)n);
    w.sums_v = (int32_t*)c.take((size_t)2 * (w.nb + 1) * 4);
    w.sums_t = w.sums_v ? w.sums_v + (w.nb + 1) : nullptr;
    w.total = c.total();
    return w;
}

}  // namespace

extern "C" {

size_t durf_mesh_workspace_bytes(int nu, int nv, int nw) {
    if (!lattice_shape_ok(nu, nv, nw, DURF_MESH_MAX_POINTS)) return 0;
    return carve_mesh(nullptr, nu * nv * nw).total;
}

int durf_mesh_count(void* stream, int nu, int nv, int nw, const float* density, const uint8_t* valid, float iso, void* workspace,
                    size_t workspace_bytes, int32_t* counts) {
    const int n = check_lattice_shape(__func__, nu, nv, nw, DURF_MESH_MAX_POINTS);
    if (n < 0) return -1;
    DURF_REQUIREF(iso == iso, "iso is a number, iso = %g", (double)iso);
    DURF_REQUIREF(density && counts, "density and counts");
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    const MeshWs w = carve_mesh(workspace, n);
    int rc = durf::check_workspace(__func__, workspace_bytes, w.total, "durf_mesh_workspace_bytes(%d, %d, %d)", nu, nv, nw);
    if (rc != 0) return rc;
    const LatticeDims D{nu, nv, nw, n};
    hipLaunchKernelGGL(k_mesh_classify, dim3(w.nb), dim3(MESH_B), 0, (hipStream_t)stream, D, density, valid, iso, w.voff, w.toff, w.mask,
                       w.sums_v, w.sums_t);
    DURF_CHECK_LAUNCH("k_mesh_classify");
    hipLaunchKernelGGL((k_scan_block_sums<int32_t, 2>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, w.nb, w.sums_v, counts);
    DURF_CHECK_LAUNCH("k_scan_block_sums<int32_t, 2>");
    hipLaunchKernelGGL(k_mesh_offsets, dim3(w.nb), dim3(MESH_B), 0, (hipStream_t)stream, n, w.voff, w.toff, w.sums_v, w.sums_t);
    DURF_CHECK_LAUNCH("k_mesh_offsets");
    return 0;
}

int durf_mesh_emit(void* stream, int nu, int nv, int nw, const float* density, const uint8_t* valid, float iso, const float* origin_host,
                   const float* du_host, const float* dv_host, const float* dw_host, const float* normal_xform_host, int flip,
                   const void* workspace, size_t workspace_bytes, int max_vertices, int max_triangles, float* vertices, float* normals,
                   int32_t* vertex_edge, float* vertex_t, int32_t* triangles) {
    const int n = check_lattice_shape(__func__, nu, nv, nw, DURF_MESH_MAX_POINTS);
    if (n < 0) return -1;
    DURF_REQUIREF(iso == iso, "iso is a number, iso = %g", (double)iso);
    DURF_REQUIREF(density != nullptr, "density");
    DURF_REQUIREF(origin_host && du_host && dv_host && dw_host, "origin, du, dv and dw");
    DURF_REQUIREF(!normals || normal_xform_host, "normals need normal_xform");
    DURF_REQUIREF(max_vertices >= 0 && max_triangles >= 0, "capacities >= 0, max_vertices = %d, max_triangles = %d", max_vertices,
                 max_triangles);
    DURF_REQUIREF(vertices || max_vertices == 0, "vertices for max_vertices = %d", max_vertices);
    DURF_REQUIREF(triangles || max_triangles == 0, "triangles for max_triangles = %d", max_triangles);
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    const MeshWs w = carve_mesh(const_cast<void*>(workspace), n);
    int rc = durf::check_workspace(__func__, workspace_bytes, w.total, "durf_mesh_workspace_bytes(%d, %d, %d)", nu, nv, nw);
    if (rc != 0) return rc;
    if (max_vertices == 0 && max_triangles == 0) return 0;
    const LatticeFrame F = lattice_frame(origin_host, du_host, dv_host, dw_host);
    MeshNormals M{};
    if (normals)
        for (int c = 0; c < 9; c++) M.A[c] = normal_xform_host[c];
    const LatticeDims D{nu, nv, nw, n};
    hipLaunchKernelGGL(k_mesh_emit, dim3(w.nb), dim3(MESH_B), 0, (hipStream_t)stream, D, density, valid, iso, F, M, flip != 0 ? 1 : 0, w.voff,
                       w.toff, w.mask, max_vertices, max_triangles, max_vertices ? vertices : nullptr, max_vertices ? normals : nullptr,
                       max_vertices ? vertex_edge : nullptr, max_vertices ? vertex_t : nullptr, triangles);
    DURF_CHECK_LAUNCH("k_mesh_emit");
    return 0;
}

int durf_mesh_gather(void* stream, int nu, int nv, int nw, const int32_t* counts, int max_vertices, const int32_t* vertex_edge,
                     const float* vertex_t, int C, const float* attr_f, float* out_f, const int32_t* attr_i, const float* density,
                     const uint8_t* valid, float iso, int32_t* out_i) {
    const int n = check_lattice_shape(__func__, nu, nv, nw, DURF_MESH_MAX_POINTS);
    if (n < 0) return -1;
    DURF_REQUIREF(max_vertices >= 0, "max_vertices >= 0, max_vertices = %d", max_vertices);
    DURF_REQUIREF(counts && vertex_edge && vertex_t, "counts, vertex_edge and vertex_t");
    DURF_REQUIREF(attr_f || attr_i, "at least one attribute");
    DURF_REQUIREF(!attr_f || (out_f && C >= 1), "attr_f needs out_f and C >= 1, C = %d", C);
    DURF_REQUIREF(!attr_i || (out_i && density), "attr_i needs out_i and density");
    DURF_REQUIREF(!attr_i || iso == iso, "iso is a number, iso = %g", (double)iso);
    if (max_vertices == 0) return 0;
    const LatticeDims D{nu, nv, nw, n};
    hipLaunchKernelGGL(k_mesh_gather, dim3(durf_cdiv((size_t)max_vertices, MESH_B)), dim3(MESH_B), 0, (hipStream_t)stream, D, counts,
                       max_vertices, vertex_edge, vertex_t, C, attr_f, out_f, attr_i, density, valid, iso, out_i);
    DURF_CHECK_LAUNCH("k_mesh_gather");
    return 0;
}

}  // extern "C"
