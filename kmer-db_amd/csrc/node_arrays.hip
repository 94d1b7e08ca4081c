// node_arrays.hip — the node arrays of the v1 kernels (a2a_v1.hip) and of new2all / db2db, derived on the device from the compact layout on
// first use (kmdb_ensure_v1_arrays, engine_state.h): {n, l, last id, stream bits} and the absolute stream position of every node, the prefix
// sums of the weights, the segments of the v1 kernels, and the list index — checkpoints of the long local lists.
#include "device_common.h"
#include "engine_state.h"
#include "prim.h"

#include <algorithm>
#include <vector>

namespace {

__global__ void v1_arrays_kernel(const uint2* __restrict__ k0in, const uint32_t* __restrict__ bitrel, const uint64_t* __restrict__ blkbase,
                                 const uint32_t* __restrict__ nl, uint32_t P, uint4* __restrict__ meta, uint64_t* __restrict__ bitpos) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint2 km = k0in[i];
    const uint32_t v = nl[i];
    meta[i] = make_uint4(v, kmdb_k0_l(km), kmdb_k0_last(km), kmdb_k0_bits(km));
    bitpos[i] = blkbase[i >> 8] + bitrel[i];
}

}  // namespace

// list index for new2all / db2db (engine_state.h): checkpoints of the long local lists
__global__ void ck_count_kernel(const uint2* __restrict__ k0in, uint32_t P, uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > P) return;
    const uint32_t l = i < P ? kmdb_k0_l(k0in[i]) : 0u;
    cnt[i] = l > KMDB_CK_IDS ? (l + KMDB_CK_IDS - 1u) / KMDB_CK_IDS : 0u;
}
__global__ void ck_fill_kernel(const uint2* __restrict__ k0in, const uint32_t* __restrict__ bitrel, const uint64_t* __restrict__ blkbase,
                               const uint64_t* __restrict__ bits, uint32_t P, const uint32_t* __restrict__ ck_ofs, uint64_t* __restrict__ ck_bit,
                               uint32_t* __restrict__ ck_id) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint2 km = k0in[i];
    const uint32_t l = kmdb_k0_l(km), last = kmdb_k0_last(km);
    if (l <= KMDB_CK_IDS) return;
    const uint64_t pos = blkbase[i >> 8] + bitrel[i];
    uint32_t id = gamma_first_id<2, false>(bits, pos, l, last), o = ck_ofs[i];
    GammaCursor<2> c(bits, pos);
    for (uint32_t t = 0; t < l; ++t) {
        if (t % KMDB_CK_IDS == 0) { ck_id[o] = id; ck_bit[o] = c.pos(); ++o; }      // element t and the position of the code after it
        if (t + 1 < l) id += c.next();
    }
}

static int ensure_v1_impl(kmdb_db* db);
int kmdb_ensure_v1_arrays(kmdb_db* db) {
    if (db->v1_ready) return 0;
    if (ensure_v1_impl(db)) {
        // nothing half made is left behind: the next call starts over
        dev_reset(db->meta, db->bitpos, db->wprefix, db->v1_counters, db->segs, db->v1_scan_tmp, db->ck_ofs, db->ck_bit, db->ck_id);
        return 1;
    }
    db->v1_ready = true;
    return 0;
}
static int ensure_v1_impl(kmdb_db* db) {
    const uint64_t P = db->P;
    DEV_ALLOC(db->meta, std::max<uint64_t>(P, 1));
    DEV_ALLOC(db->bitpos, std::max<uint64_t>(P, 1));
    DEV_ALLOC(db->wprefix, P + 1);
    DEV_ALLOC(db->v1_counters, 8);
    HIP_TRY(hipMemset(db->v1_counters, 0, 8 * sizeof(unsigned long long)));
    if (P) hipLaunchKernelGGL(v1_arrays_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, db->stream, db->k0in, db->bitrel, db->blkbase, db->nl,
                              (uint32_t)P, db->meta, db->bitpos);
    HIP_TRY(hipGetLastError());
    std::vector<Segment> segs;
    const uint64_t step = 2048;
    for (uint64_t f = 0; f < P; f += step) segs.push_back(Segment{(uint32_t)f, (uint32_t)std::min<uint64_t>(P, f + step)});
    while (segs.size() % WAVES_PER_BLOCK) segs.push_back(Segment{(uint32_t)P, (uint32_t)P});
    DEV_ALLOC(db->segs, std::max<size_t>(segs.size(), 1));
    if (!segs.empty()) HIP_TRY(hipMemcpy(db->segs, segs.data(), segs.size() * sizeof(Segment), hipMemcpyHostToDevice));
    db->n_segs = (uint32_t)segs.size();
    HIP_TRY(prim::exclusive_sum(nullptr, db->v1_scan_tmp_bytes, db->w.get(), db->wprefix.get(), (int)(P + 1)));
    DEV_ALLOC(db->v1_scan_tmp, std::max<size_t>(db->v1_scan_tmp_bytes, 16));
    {
        const uint64_t P1 = P + 1;
        DevBuf<uint32_t> cnt;
        DevBuf<void> tmp;
        size_t tb = 0;
        DEV_ALLOC(cnt, P1);
        DEV_ALLOC(db->ck_ofs, P1);
        hipLaunchKernelGGL(ck_count_kernel, dim3((unsigned)((P1 + 255) / 256)), dim3(256), 0, db->stream, db->k0in, (uint32_t)P, cnt);
        HIP_TRY(prim::exclusive_sum(nullptr, tb, cnt.get(), db->ck_ofs.get(), (int)P1, db->stream));
        DEV_ALLOC(tmp, std::max<size_t>(tb, 16));
        HIP_TRY(prim::exclusive_sum(tmp, tb, cnt.get(), db->ck_ofs.get(), (int)P1, db->stream));
        uint32_t n_ck = 0;
        HIP_TRY(hipMemcpyAsync(&n_ck, db->ck_ofs + P, 4, hipMemcpyDeviceToHost, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));
        cnt.reset(); tmp.reset();
        DEV_ALLOC(db->ck_bit, std::max<uint64_t>(n_ck, 1));
        DEV_ALLOC(db->ck_id, std::max<uint64_t>(n_ck, 1));
        if (P) hipLaunchKernelGGL(ck_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, db->stream, db->k0in, db->bitrel, db->blkbase, db->bits,
                                  (uint32_t)P, db->ck_ofs, db->ck_bit, db->ck_id);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(db->stream));
    return 0;
}
