// grad_tables.hpp -- the tables of grad_fused.hpp's GradTables for one factor list, built on the host from plain arrays: the
// list cut into chunks and tiles, a tile's cameras numbered, a chunk's entries ranked by camera and by point block, per block
// the choice between "straight to g" and staging slots, the variables no listed factor reads.  The order in which the fused
// gradient adds follows these tables.  Pure integer work: no HIP call, no problem, no environment (rdis_hip.hip's
// build_grad_plan picks the tile size, calls this, allocates and uploads); tests/cpp/grad_tables_test.cpp runs it without a
// device and tests/test_grad_tables_cpu.py walks its tables as grad_fused.hip's kernels do.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>
#include "host_blocks.hpp"

namespace rdis_hip {

constexpr unsigned short GRAD_TABLES_NO_ENTRY = 0xFFFF;   // grad_fused.hpp: GRAD_NO_ENTRY (rdis_hip.hip asserts them equal)

struct IntPair { int x, y; };   // the tables' pairs, on the device an int2 (rdis_hip.hip asserts the layout)

struct GradIndex {
    int nchunks = 0, ntiles = 0, ncam_cap = 1;   // chunks of the list; tiles; the largest number of distinct cameras in a tile
    int ncs = 0, nps = 0, nz = 0;                // staged camera blocks, staged point blocks, untouched variables
    int cstage_slots = 0, pstage_slots = 0;      // slots of the camera / point staging array
    // one int32 block: ptv | tile_chunk0 | tile_cam0 | tile_cam | chunk_cseg0 | cseg | chunk_pseg0 | pseg | cs_var | cs_ptr |
    // ps_var | ps_ptr | zvar, each padded to an even number of entries (the pairs stay 8-byte aligned)
    ivec blk;
    size_t o_ptv = 0, o_tc0 = 0, o_tm0 = 0, o_tcam = 0, o_cs0 = 0, o_cseg = 0, o_ps0 = 0, o_pseg = 0, o_csv = 0, o_csp = 0,
           o_psv = 0, o_psp = 0, o_z = 0;
    // one 16-bit block: cl | rc | rp, npad entries each (the list padded to whole chunks)
    std::vector<unsigned short> sh;
    size_t npad = 0;
};

// Everything here is index work over the list:
// cut it into chunks and tiles, number a tile's cameras, rank a chunk's entries by camera and by point block (list order
// within a block: the order of the sums), decide per block whether one chunk / tile holds all its listed factors (straight to
// g) or several do (a staging slot each, a block's slots consecutive in chunk / tile order).
// cam, pt: [F] a factor's camera and point block (first variable ids); cam_ord: [N] ordinal of the camera block that starts at
// a variable id; fac: [nf] the list, or null = 0 .. nf-1; GW: entries of a chunk; tile_chunks: chunks of a tile, fewer where
// their cameras would exceed cam_soft.
inline void grad_tables_build(size_t N, size_t ncb, const int* cam, const int* pt, const int* cam_ord, int nf, const int64_t* fac,
                              int GW, int tile_chunks, int cam_soft, GradIndex& T) {
    const int nchunks = (nf + GW - 1) / GW;
    auto fid_of = [&](int j) { return fac ? (int)fac[j] : j; };
    // how many listed factors read each block
    ivec cnt_cam(ncb, 0), cnt_pt(N, 0);
    for (int j = 0; j < nf; ++j) { const int f = fid_of(j); ++cnt_cam[(size_t)cam_ord[(size_t)cam[(size_t)f]]]; ++cnt_pt[(size_t)pt[(size_t)f]]; }
    // tiles: up to tile_chunks chunks, fewer where their cameras would not fit (a chunk alone always does)
    const size_t npad = (size_t)nchunks * GW;
    std::vector<unsigned short>& sh = T.sh;   // cl | rc | rp
    sh.assign(3 * npad, GRAD_TABLES_NO_ENTRY);
    unsigned short* const cl = sh.data();
    unsigned short* const rc = cl + npad;
    unsigned short* const rp = rc + npad;
    ivec ptv(npad, 0), tile_chunk0, tile_cam0, chunk_cseg0((size_t)nchunks + 1, 0), chunk_pseg0((size_t)nchunks + 1, 0);
    std::vector<IntPair> tile_cam, cseg, pseg;
    ivec cam_tile(ncb, -1), cam_local(ncb, 0);           // camera ordinal -> tile it was last numbered in, its number there
    ivec tcnt;                                            // listed factors of a tile's camera inside the tile
    std::vector<std::pair<int, int>> cstaged, pstaged;    // (block, index of the table entry to patch), in tile / chunk order
    ivec pt_chunk(N, -1), pt_seg(N, 0);                   // point block -> chunk it was last seen in, its segment there
    ivec segcnt, segrow, seg_of((size_t)GW), cam_seg_chunk, cam_seg;
    int ncam_cap = 1;
    tile_chunk0.push_back(0); tile_cam0.push_back(0);
    for (int ch0 = 0; ch0 < nchunks;) {
        const int tile = (int)tile_chunk0.size() - 1;
        const size_t tc0 = tile_cam.size();
        int ch1 = ch0;
        while (ch1 < nchunks && ch1 - ch0 < tile_chunks) {
            // the cameras this chunk would add
            const size_t before = tile_cam.size();
            const int j0 = ch1 * GW, j1 = std::min(nf, j0 + GW);
            for (int j = j0; j < j1; ++j) {
                const int o = cam_ord[(size_t)cam[(size_t)fid_of(j)]];
                if (cam_tile[(size_t)o] != tile) { cam_tile[(size_t)o] = tile; cam_local[(size_t)o] = (int)(tile_cam.size() - tc0); tile_cam.push_back(IntPair{o, 0}); }
            }
            if (ch1 > ch0 && tile_cam.size() - tc0 > (size_t)cam_soft) {   // too many: the chunk starts the next tile
                for (size_t k = before; k < tile_cam.size(); ++k) cam_tile[(size_t)tile_cam[k].x] = -1;
                tile_cam.resize(before);
                break;
            }
            ++ch1;
        }
        const int nc = (int)(tile_cam.size() - tc0);
        ncam_cap = std::max(ncam_cap, nc);
        tcnt.assign((size_t)nc, 0);
        cam_seg_chunk.assign((size_t)nc, -1); cam_seg.assign((size_t)nc, 0);
        for (int ch = ch0; ch < ch1; ++ch) {
            const int j0 = ch * GW, j1 = std::min(nf, j0 + GW);
            // segments by camera, in order of first appearance; list order within a segment
            segcnt.clear();
            for (int j = j0; j < j1; ++j) {
                const int f = fid_of(j);
                const int l = cam_local[(size_t)cam_ord[(size_t)cam[(size_t)f]]];
                cl[j] = (unsigned short)l;
                ptv[(size_t)j] = pt[(size_t)f];
                ++tcnt[(size_t)l];
                if (cam_seg_chunk[(size_t)l] != ch) { cam_seg_chunk[(size_t)l] = ch; cam_seg[(size_t)l] = (int)segcnt.size(); segcnt.push_back(0); cseg.push_back(IntPair{l, 0}); }
                seg_of[(size_t)(j - j0)] = cam_seg[(size_t)l];
                ++segcnt[(size_t)cam_seg[(size_t)l]];
            }
            {
                const size_t s0 = cseg.size() - segcnt.size();
                segrow.assign(segcnt.size() + 1, 0);
                for (size_t k = 0; k < segcnt.size(); ++k) { segrow[k + 1] = segrow[k] + segcnt[k]; cseg[s0 + k].y = segrow[k]; }
                for (int j = j0; j < j1; ++j) rc[j] = (unsigned short)segrow[(size_t)seg_of[(size_t)(j - j0)]]++;
                cseg.push_back(IntPair{0, j1 - j0});
                chunk_cseg0[(size_t)ch + 1] = (int)cseg.size();
            }
            // ... and by point block
            segcnt.clear();
            for (int j = j0; j < j1; ++j) {
                const int q = ptv[(size_t)j];
                if (pt_chunk[(size_t)q] != ch) { pt_chunk[(size_t)q] = ch; pt_seg[(size_t)q] = (int)segcnt.size(); segcnt.push_back(0); pseg.push_back(IntPair{q, 0}); }
                seg_of[(size_t)(j - j0)] = pt_seg[(size_t)q];
                ++segcnt[(size_t)pt_seg[(size_t)q]];
            }
            {
                const size_t s0 = pseg.size() - segcnt.size();
                segrow.assign(segcnt.size() + 1, 0);
                for (size_t k = 0; k < segcnt.size(); ++k) {
                    segrow[k + 1] = segrow[k] + segcnt[k];
                    pseg[s0 + k].y = segrow[k];
                    // all the block's listed factors in this chunk: its sum goes straight to g (destination = its id, as set)
                    if (segcnt[k] != cnt_pt[(size_t)pseg[s0 + k].x]) pstaged.emplace_back(pseg[s0 + k].x, (int)(s0 + k));
                }
                for (int j = j0; j < j1; ++j) rp[j] = (unsigned short)segrow[(size_t)seg_of[(size_t)(j - j0)]]++;
                pseg.push_back(IntPair{0, j1 - j0});
                chunk_pseg0[(size_t)ch + 1] = (int)pseg.size();
            }
        }
        for (int l = 0; l < nc; ++l) {
            IntPair& e = tile_cam[tc0 + (size_t)l];
            const int o = e.x;
            if (tcnt[(size_t)l] == cnt_cam[(size_t)o]) e.y = -1;   // (patched below: the block's first variable id)
            else { e.y = -2; cstaged.emplace_back(o, (int)(tc0 + (size_t)l)); }
        }
        tile_chunk0.push_back(ch1);
        tile_cam0.push_back((int)tile_cam.size());
        ch0 = ch1;
    }
    // camera ordinal -> first variable id
    ivec cam_first(ncb, 0);
    for (size_t v = 0; v < N; ++v) if (cam_ord[v] >= 0) cam_first[(size_t)cam_ord[v]] = (int)v;
    for (IntPair& e : tile_cam) if (e.y == -1) e.y = cam_first[(size_t)e.x];
    // staging slots: a block's partial sums consecutive, in the order they were made
    ivec cs_var, cs_ptr(1, 0), ps_var, ps_ptr(1, 0);
    {
        ivec n_of(ncb, 0), base(ncb, 0);
        for (const auto& e : cstaged) ++n_of[(size_t)e.first];
        for (size_t o = 0; o < ncb; ++o)
            if (n_of[o] > 0) { base[o] = cs_ptr.back(); cs_var.push_back(cam_first[o]); cs_ptr.push_back(cs_ptr.back() + n_of[o]); }
        for (const auto& e : cstaged) tile_cam[(size_t)e.second].y = ~(base[(size_t)e.first]++);
    }
    {
        ivec& n_of = pt_seg;    // (scratch: the per-chunk segment numbers are not needed any more)
        ivec& base = pt_chunk;
        for (const auto& e : pstaged) n_of[(size_t)e.first] = 0;
        for (const auto& e : pstaged) ++n_of[(size_t)e.first];
        ivec blocks;
        for (const auto& e : pstaged) if (n_of[(size_t)e.first] > 0) { blocks.push_back(e.first); n_of[(size_t)e.first] = -n_of[(size_t)e.first]; }
        std::sort(blocks.begin(), blocks.end());
        for (int q : blocks) { base[(size_t)q] = ps_ptr.back(); ps_var.push_back(q); ps_ptr.push_back(ps_ptr.back() - n_of[(size_t)q]); }
        for (const auto& e : pstaged) pseg[(size_t)e.second].x = ~(base[(size_t)e.first]++);
    }
    // variables no listed factor reads
    ivec zvar;
    {
        cvec touched(N, 0);
        for (size_t o = 0; o < ncb; ++o) if (cnt_cam[o] > 0) for (int k = 0; k < 9; ++k) touched[(size_t)cam_first[o] + k] = 1;
        for (size_t v = 0; v < N; ++v) if (cnt_pt[v] > 0) for (int k = 0; k < 3; ++k) touched[v + k] = 1;
        for (size_t v = 0; v < N; ++v) if (!touched[v]) zvar.push_back((int)v);
    }
    // one int32 block, one 16-bit block
    ivec& blk = T.blk;
    auto put = [&](const int* v, size_t n) { const size_t off = blk.size(); blk.insert(blk.end(), v, v + n); if (blk.size() & 1) blk.push_back(0); return off; };
    T.o_ptv = put(ptv.data(), ptv.size()); T.o_tc0 = put(tile_chunk0.data(), tile_chunk0.size()); T.o_tm0 = put(tile_cam0.data(), tile_cam0.size());
    T.o_tcam = put(reinterpret_cast<const int*>(tile_cam.data()), 2 * tile_cam.size());
    T.o_cs0 = put(chunk_cseg0.data(), chunk_cseg0.size()); T.o_cseg = put(reinterpret_cast<const int*>(cseg.data()), 2 * cseg.size());
    T.o_ps0 = put(chunk_pseg0.data(), chunk_pseg0.size()); T.o_pseg = put(reinterpret_cast<const int*>(pseg.data()), 2 * pseg.size());
    T.o_csv = put(cs_var.data(), cs_var.size()); T.o_csp = put(cs_ptr.data(), cs_ptr.size());
    T.o_psv = put(ps_var.data(), ps_var.size()); T.o_psp = put(ps_ptr.data(), ps_ptr.size());
    T.o_z = put(zvar.data(), zvar.size());
    T.npad = npad;
    T.nchunks = nchunks; T.ntiles = (int)tile_chunk0.size() - 1; T.ncam_cap = ncam_cap;
    T.ncs = (int)cs_var.size(); T.nps = (int)ps_var.size(); T.nz = (int)zvar.size();
    T.cstage_slots = cs_ptr.back(); T.pstage_slots = ps_ptr.back();
}

}  // namespace rdis_hip
