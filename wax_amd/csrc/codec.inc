// codec.inc — part of engine.hip's translation unit (included there; not compiled alone).
// C ABI: MV2V encoding-2 serialize / deserialize (MetalVectorEngine.swift:682-815)

// ---- persistence ----------------------------------------------------------

void wax_hip_free(void* p) { std::free(p); }

int wax_hip_serialize(wax_hip_engine* e, uint8_t** out_bytes, size_t* out_len) {
    if (!e || !out_bytes || !out_len) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (e->sh) return sh_serialize(e, out_bytes, out_len);
    DeviceGuard g(e->device);
    e->lock.lock_shared(holding(e) > 0);  // withReadLock (:683)
    { const int frc = flush_pending(e); if (frc != WAX_HIP_OK) { e->lock.unlock_shared(); return frc; } }
    const uint64_t n = e->count;
    const uint64_t vec_bytes = n * (uint64_t)e->dims * 4ull;  // :697
    const uint64_t id_bytes = n * 8ull;                       // :707
    const size_t total = 36 + (size_t)vec_bytes + 8 + (size_t)id_bytes;
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(total));
    if (!buf) { e->lock.unlock_shared(); return fail(WAX_HIP_ERR_ALLOC, "Failed to allocate serialize buffer"); }
    uint8_t* p = buf;
    const uint8_t magic[4] = {0x4D, 0x56, 0x32, 0x56};        // "MV2V" :686
    std::memcpy(p, magic, 4); p += 4;
    const uint16_t ver = 1; std::memcpy(p, &ver, 2); p += 2;  // :687
    *p++ = 2;                                                 // encoding 2 (flat) :689
    *p++ = e->metric;                                         // VecSimilarity raw :690
    std::memcpy(p, &e->dims, 4); p += 4;                      // :691
    std::memcpy(p, &n, 8); p += 8;                            // :693
    std::memcpy(p, &vec_bytes, 8); p += 8;                    // :698
    std::memset(p, 0, 8); p += 8;                             // reserved :700
    int rc = WAX_HIP_OK;
    if (vec_bytes) {
        hipError_t err = hipMemcpy(p, e->d_store, (size_t)vec_bytes, hipMemcpyDeviceToHost);  // :703-705
        if (err != hipSuccess) rc = fail(WAX_HIP_ERR_INTERNAL, std::string("vector download: ") + hipGetErrorString(err));
    }
    p += vec_bytes;
    std::memcpy(p, &id_bytes, 8); p += 8;                     // :708
    if (id_bytes) std::memcpy(p, e->ids.data(), (size_t)id_bytes);  // :710
    e->lock.unlock_shared();
    if (rc != WAX_HIP_OK) { std::free(buf); return rc; }
    *out_bytes = buf;
    *out_len = total;
    return WAX_HIP_OK;
}

int wax_hip_deserialize(wax_hip_engine* e, const uint8_t* data, size_t len) {
    if (!e || (!data && len)) return fail(WAX_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (e->sh) return sh_deserialize(e, data, len);
    uint64_t n = 0, vec_len = 0, id_len = 0;
    { const int vrc = validate_mv2v_segment(e->metric, e->dims, data, len, &n, &vec_len, &id_len); if (vrc != WAX_HIP_OK) return vrc; }
    REFUSE_IF_HOLDING(e);
    DeviceGuard g(e->device);
    WriteGuard w(e->lock);  // withWriteLock (:717)
    sync_shard_work(e);
    e->derived.replaced();
    e->cols.clear();          // MV2V has no field for any per-row column: every row of the loaded store holds the defaults
    e->pend_rows.store(0, std::memory_order_release);   // the store is replaced wholesale: staged appends are dropped with it
    // :790-792 — capacity only grows
    int rc = resize_store(e, n > e->capacity ? n : e->capacity);
    if (rc != WAX_HIP_OK) return rc;
    e->count = n;
    e->ids.resize((size_t)n);
    if (n) {
        std::memcpy(e->ids.data(), data + 36 + vec_len + 8, (size_t)id_len);  // :809-811
        HIP_TRY(hipMemcpy(e->d_store, data + 36, (size_t)vec_len, hipMemcpyHostToDevice), WAX_HIP_ERR_INTERNAL, "vector upload");  // :794-799
        HIP_TRY(hipMemcpy(e->d_ids, e->ids.data(), (size_t)id_len, hipMemcpyHostToDevice), WAX_HIP_ERR_INTERNAL, "frame id upload");
    }
    e->idmap.clear();
    e->idmap.reserve((size_t)n);
    for (uint64_t i = 0; i < n; ++i)
        if (e->idmap.find(e->ids[i]) < 0) e->idmap.put(e->ids[i], (uint32_t)i);  // firstIndex(of:) semantics: first row wins
    return WAX_HIP_OK;
}

