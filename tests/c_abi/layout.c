/* What a C compiler makes of include/wax_hip.h: the size of every struct the header defines, the offset and size of every member,
 * and the value of every constant that wax_amd/_abi.py restates. tests/test_c_boundary_cpu.py compares each line with _abi's
 * ctypes.Structure fields and constants. Plain C11; needs neither the library nor a device.
 *
 *   struct <name> <size>
 *   field <struct> <member> <offset> <size>
 *   const <NAME> <value>            (signed values as %lld, the UINT64_MAX sentinels as %llu) */
#include <stddef.h>
#include <stdio.h>

#include "wax_hip.h"

#define STRUCT(T) printf("struct %s %zu\n", #T, sizeof(T))
#define FIELD(T, m) printf("field %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T*)0)->m))
#define CONST_I(name) printf("const %s %lld\n", #name, (long long)(name))
#define CONST_U(name) printf("const %s %llu\n", #name, (unsigned long long)(name))

int main(void) {
    STRUCT(wax_hip_hit);
    FIELD(wax_hip_hit, key);
    FIELD(wax_hip_hit, frame_id);

    STRUCT(wax_hip_stats_t);
    FIELD(wax_hip_stats_t, searches);
    FIELD(wax_hip_stats_t, rows_scanned);
    FIELD(wax_hip_stats_t, bytes_scanned);
    FIELD(wax_hip_stats_t, transient_allocations);
    FIELD(wax_hip_stats_t, reuse_count);
    FIELD(wax_hip_stats_t, reserved_rows);
    FIELD(wax_hip_stats_t, last_scan_kernel_ms);
    FIELD(wax_hip_stats_t, scan_kernel_ms_total);
    FIELD(wax_hip_stats_t, scan_kernels_timed);
    FIELD(wax_hip_stats_t, batch_gemm_ms_total);
    FIELD(wax_hip_stats_t, batch_gemms_timed);
    FIELD(wax_hip_stats_t, batch_gemm_rows);
    FIELD(wax_hip_stats_t, batch_gemm_queries);

    STRUCT(wax_hip_rrf_lane);
    FIELD(wax_hip_rrf_lane, d_ids);
    FIELD(wax_hip_rrf_lane, d_counts);
    FIELD(wax_hip_rrf_lane, stride);
    FIELD(wax_hip_rrf_lane, pitch);
    FIELD(wax_hip_rrf_lane, weight);

    STRUCT(wax_hip_row_predicate);
    FIELD(wax_hip_row_predicate, has_after);
    FIELD(wax_hip_row_predicate, after);
    FIELD(wax_hip_row_predicate, has_before);
    FIELD(wax_hip_row_predicate, before);
    FIELD(wax_hip_row_predicate, deny_flags);

    STRUCT(wax_hip_predicate_ticket_stats_t);
    FIELD(wax_hip_predicate_ticket_stats_t, submitted);
    FIELD(wax_hip_predicate_ticket_stats_t, rode);
    FIELD(wax_hip_predicate_ticket_stats_t, masked_passes);
    FIELD(wax_hip_predicate_ticket_stats_t, certified);
    FIELD(wax_hip_predicate_ticket_stats_t, fallbacks);
    FIELD(wax_hip_predicate_ticket_stats_t, deferred);
    FIELD(wax_hip_predicate_ticket_stats_t, host_decided);
    FIELD(wax_hip_predicate_ticket_stats_t, bitmap_builds);
    FIELD(wax_hip_predicate_ticket_stats_t, bitmap_hits);

    STRUCT(wax_hip_group_stats_t);
    FIELD(wax_hip_group_stats_t, searches);
    FIELD(wax_hip_group_stats_t, fused_scans);
    FIELD(wax_hip_group_stats_t, column_scans);
    FIELD(wax_hip_group_stats_t, member_rounds);
    FIELD(wax_hip_group_stats_t, group_slots);
    FIELD(wax_hip_group_stats_t, parent_rows_uploaded);

    STRUCT(wax_hip_term_stats_t);
    FIELD(wax_hip_term_stats_t, searches);
    FIELD(wax_hip_term_stats_t, device_masks);
    FIELD(wax_hip_term_stats_t, host_staged);
    FIELD(wax_hip_term_stats_t, host_decided);
    FIELD(wax_hip_term_stats_t, term_rows_uploaded);
    FIELD(wax_hip_term_stats_t, term_values_uploaded);

    STRUCT(wax_hip_term_batch_stats_t);
    FIELD(wax_hip_term_batch_stats_t, calls);
    FIELD(wax_hip_term_batch_stats_t, queries);
    FIELD(wax_hip_term_batch_stats_t, sets);
    FIELD(wax_hip_term_batch_stats_t, mask_launches);
    FIELD(wax_hip_term_batch_stats_t, looped);
    FIELD(wax_hip_term_batch_stats_t, host_decided);

    CONST_I(WAX_HIP_ABI_VERSION);
    CONST_I(WAX_HIP_OK);
    CONST_I(WAX_HIP_ERR_DIM_MISMATCH);
    CONST_I(WAX_HIP_ERR_CAPACITY);
    CONST_I(WAX_HIP_ERR_NO_DEVICE);
    CONST_I(WAX_HIP_ERR_ALLOC);
    CONST_I(WAX_HIP_ERR_BAD_SEGMENT);
    CONST_I(WAX_HIP_ERR_METRIC_UNSUPPORTED);
    CONST_I(WAX_HIP_ERR_INVALID_ARGUMENT);
    CONST_I(WAX_HIP_ERR_INTERNAL);
    CONST_I(WAX_HIP_METRIC_COSINE);
    CONST_I(WAX_HIP_METRIC_DOT);
    CONST_I(WAX_HIP_METRIC_L2);
    CONST_I(WAX_HIP_MAX_RESULTS);
    CONST_I(WAX_HIP_FLAG_DELETED);
    CONST_I(WAX_HIP_FLAG_SUPERSEDED);
    CONST_I(WAX_HIP_FLAG_SURROGATE);
    CONST_I(WAX_HIP_FLAG_USER_SHIFT);
    CONST_I(WAX_HIP_GROUP_MAX_LIMIT);
    CONST_I(WAX_HIP_GROUP_MAX_MEMBERS);
    CONST_I(WAX_HIP_TERMS_MAX_PER_ROW);
    CONST_I(WAX_HIP_TERMS_MAX_REQUIRED);
    CONST_U(WAX_HIP_NO_ALLOW_LIST);
    CONST_U(WAX_HIP_NO_PARENT);
    return 0;
}
