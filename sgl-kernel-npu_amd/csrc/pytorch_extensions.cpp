// torch.ops.npu.* registry for MI355X.
// Mirrors the reference registration unit csrc/pytorch_extensions.cpp (schemas :24-201 under TORCH_LIBRARY_FRAGMENT(npu, m),
// implementations :205-316) for the hot-path operators: the namespace stays `npu` so SGLang's call sites
// (`torch.ops.npu.<op>`) are unchanged; the dispatch key is CUDA (= HIP on ROCm) instead of PrivateUse1.
// The implementations are thin host functions (namespace sglang::npu_kernel, like include/sgl_kenel_npu_ops.h:14-239)
// that validate arguments, allocate outputs and call the C-ABI of include/mi_sgl_kernels.h on the current stream.
#include <cstdlib>
#include <map>
#include <mutex>

#include <hip/hip_runtime_api.h>
#include <ATen/ATen.h>
#include <c10/util/string_view.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "mi_sgl_kernels.h"

namespace sglang {
namespace npu_kernel {

static void *cur_stream() { return (void *)c10::hip::getCurrentHIPStream().stream(); }

static int dtype_code(const at::Tensor &t)
{
    TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf, "expected a bfloat16 / float16 tensor, got ",
                t.scalar_type());
    return t.scalar_type() == at::kBFloat16 ? MI_DTYPE_BF16 : MI_DTYPE_F16;
}

static int dtype_code3(const at::Tensor &t)        // the row statistics / scalings also take fp32 (the reference tests run them in fp32)
{
    if (t.scalar_type() == at::kFloat) return MI_DTYPE_F32;
    return dtype_code(t);
}

std::string sgl_kernel_npu_version() { return std::string("sgl-kernel-npu_amd 0.1 (") + mi_sgl_kernels_version() + ")"; }

at::Tensor decode_mla_plan(const at::Tensor &kv_seq_lens, int64_t num_kv_heads);
void decode_mla_planned(const at::Tensor &q, const at::Tensor &k_nope_buffer, const at::Tensor &k_rope_buffer, at::Tensor &att_out,
                        const at::Tensor &kv_seq_lens, double sm_scale, int64_t page_size, const at::Tensor &block_table, const at::Tensor &plan);

// The attention layers of a decode step call decode_mla with the SAME kv_seq_lens tensor: the work list of the planned form is built by
// the first of them and reused by the others (the reference signature has no plan argument, so a drop-in caller gets "plan once, run
// many" this way).  One entry per device: a WEAK reference to the kv_seq_lens tensor's storage (the entry pins neither the tensor nor its
// allocator block: when the caller drops the tensor -- a model reload -- the reference expires and the next call rebuilds; while it is
// alive the bytes cannot have been recycled for another tensor; views of one buffer -- a padded kv_seq_lens cut to the batch -- share it), its data pointer and version counter (an in-place write through torch rebuilds
// the list), kv head count and stream.  Writes that bypass the version counter (a raw-pointer kernel, a graph replay) leave a stale list
// in place -- which the kernels tolerate by construction (pieces are clamped to the current lengths, the last piece runs to their end):
// stale costs balance, never correctness.  Inference tensors carry no version counter and are not cached.  MI_MLA_PLAN_CACHE=0 turns the
// reuse off; num_splits = -1 asks for the planned form with a list of its own; torch.ops.npu.clear_mla_plan_cache() drops every entry
// (the only thing an entry owns is its list: batch * kv_heads * 8 B + 1 KB of device memory).
struct MlaPlanCacheEntry {
    c10::weak_intrusive_ptr<c10::StorageImpl> lens{c10::intrusive_ptr<c10::StorageImpl>()};
    const void *lens_ptr = nullptr;
    int64_t lens_numel = 0;
    at::Tensor plan;
    uint32_t version = 0;
    int64_t kv_heads = 0;
    void *stream = nullptr;
    unsigned long long capture = 0;      // id of the stream capture the list was built in (0: built eagerly)
};
static std::mutex g_plan_mu;
static std::map<int, MlaPlanCacheEntry> &plan_entries()
{
    static auto &entries = *new std::map<int, MlaPlanCacheEntry>();      // (never destroyed: tensors must not outlive the HIP context at exit)
    return entries;
}
void clear_mla_plan_cache()
{
    std::lock_guard<std::mutex> lk(g_plan_mu);
    plan_entries().clear();
}
static at::Tensor cached_mla_plan(const at::Tensor &kv_seq_lens, int64_t kv_heads)
{
    void *st = cur_stream();
    const uint32_t ver = kv_seq_lens._version();
    // a list built while a graph is being captured has no contents until the graph runs: it serves the calls of the SAME capture only (the
    // layers of the captured step), never an eager call or another capture
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    unsigned long long cap = 0;
    if (hipStreamGetCaptureInfo((hipStream_t)st, &cap_status, &cap) != hipSuccess) {
        (void)hipGetLastError();         // a failed query must not sit in the thread's last-error slot: the plan launch checks it right after
        cap = 0;
    } else if (cap_status != hipStreamCaptureStatusActive) {
        cap = 0;
    }
    std::lock_guard<std::mutex> lk(g_plan_mu);
    MlaPlanCacheEntry &e = plan_entries()[kv_seq_lens.device().index()];
    // same storage, still alive (expired once the caller dropped every tensor on it), same bytes, unmodified through torch
    const bool alive = e.lens_ptr != nullptr && e.lens._unsafe_get_target() == kv_seq_lens.storage().unsafeGetStorageImpl() && !e.lens.expired();
    if (alive && e.lens_ptr == kv_seq_lens.data_ptr() && e.lens_numel == kv_seq_lens.numel() && e.version == ver &&
        e.kv_heads == kv_heads && e.stream == st && e.capture == cap)
        return e.plan;
    e.plan = decode_mla_plan(kv_seq_lens, kv_heads);
    e.lens = kv_seq_lens.storage().getWeakStorageImpl();
    e.lens_ptr = kv_seq_lens.data_ptr(), e.lens_numel = kv_seq_lens.numel();
    e.version = ver, e.kv_heads = kv_heads, e.stream = st, e.capture = cap;
    return e.plan;
}

// Paged MLA decode, same argument meaning as the reference Python entry point decode_mla
// (python/sgl_kernel_npu/sgl_kernel_npu/attention/decode_attention.py:166-175); writes att_out in place.
void decode_mla(const at::Tensor &q, const at::Tensor &k_nope_buffer, const at::Tensor &k_rope_buffer, at::Tensor &att_out,
                const at::Tensor &kv_seq_lens, double sm_scale, int64_t page_size, const at::Tensor &block_table,
                int64_t num_splits)
{
    const c10::DeviceGuard device_guard(q.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(q.dim() == 3 && k_nope_buffer.dim() == 4 && k_rope_buffer.dim() == 4 && att_out.dim() == 3 && block_table.dim() == 2,
                "decode_mla: bad ranks");
    TORCH_CHECK(k_nope_buffer.size(3) == 512 && k_rope_buffer.size(3) == 64 && q.size(2) == 576 && att_out.size(2) == 512,
                "decode_mla: this build supports the MLA head layout 512 (nope) + 64 (rope)");
    TORCH_CHECK(q.stride(2) == 1 && k_nope_buffer.stride(3) == 1 && k_rope_buffer.stride(3) == 1 && att_out.stride(2) == 1,
                "decode_mla: innermost dimension must be contiguous");
    TORCH_CHECK(k_nope_buffer.size(1) == page_size && k_rope_buffer.size(1) == page_size, "decode_mla: page_size mismatch");
    TORCH_CHECK(q.scalar_type() == k_nope_buffer.scalar_type() && q.scalar_type() == k_rope_buffer.scalar_type() &&
                    q.scalar_type() == att_out.scalar_type(), "decode_mla: dtype mismatch");
    TORCH_CHECK(kv_seq_lens.scalar_type() == at::kInt && block_table.scalar_type() == at::kInt && kv_seq_lens.is_contiguous(),
                "decode_mla: kv_seq_lens / block_table must be int32");
    TORCH_CHECK(block_table.stride(1) == 1, "decode_mla: block_table rows must be contiguous");
    const int B = (int)q.size(0), Hq = (int)q.size(1), Hkv = (int)k_nope_buffer.size(2);
    TORCH_CHECK(Hq % Hkv == 0 && k_rope_buffer.size(2) == Hkv, "decode_mla: head counts");
    // The batch is q's (as in the reference, decode_attention.py:178); a longer (padded, graph-static) kv_seq_lens is cut to it HERE: the
    // work list's item offsets depend on the (sequence, kv head) pair count, so list builder and consumers must agree on it.
    TORCH_CHECK(kv_seq_lens.dim() == 1 && kv_seq_lens.size(0) >= B, "decode_mla: kv_seq_lens must be [batch] with batch >= q.size(0)");
    if (kv_seq_lens.size(0) > B) {
        decode_mla(q, k_nope_buffer, k_rope_buffer, att_out, kv_seq_lens.narrow(0, 0, B), sm_scale, page_size, block_table, num_splits);
        return;
    }
    const int max_len = (int)std::min<int64_t>(block_table.size(1) * page_size, INT32_MAX);   // upper bound, no host sync
    int splits = (int)num_splits;
    if (splits == 0) {
        splits = mi_mla_decode_num_splits(B, Hq, Hkv, max_len);
        static const bool reuse = !(getenv("MI_MLA_PLAN_CACHE") && atoi(getenv("MI_MLA_PLAN_CACHE")) == 0);
        if (splits == MI_MLA_SPLITS_PLANNED && reuse && B > 0 && !kv_seq_lens.is_inference()) {
            decode_mla_planned(q, k_nope_buffer, k_rope_buffer, att_out, kv_seq_lens, sm_scale, page_size, block_table, cached_mla_plan(kv_seq_lens, Hkv));
            return;
        }
    }
    const size_t wsb = mi_mla_decode_workspace(B, Hq, splits);
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(q.device()));
    const int rc = mi_mla_decode(q.data_ptr(), k_nope_buffer.data_ptr(), k_rope_buffer.data_ptr(), att_out.data_ptr(),
                                 kv_seq_lens.data_ptr<int>(), block_table.data_ptr<int>(), B, Hq, Hkv, (int)page_size,
                                 (int)block_table.stride(0), max_len, q.stride(0), q.stride(1), k_nope_buffer.stride(0),
                                 k_nope_buffer.stride(1), k_nope_buffer.stride(2), k_rope_buffer.stride(0),
                                 k_rope_buffer.stride(1), k_rope_buffer.stride(2), att_out.stride(0), att_out.stride(1),
                                 (float)sm_scale, dtype_code(q), splits, ws.data_ptr(), wsb, cur_stream());
    TORCH_CHECK(rc == 0, "mi_mla_decode failed with code ", rc);
}

// MI355X extension (plan once, run many): the length-aware work list of decode_mla depends only on kv_seq_lens -- the attention layers of a
// decode step share it.  decode_mla_plan builds it (one small launch, no host sync); decode_mla_planned is decode_mla with that list
// instead of a plan launch of its own.  Where the planned form does not serve the shape, the planned call runs plain decode_mla.
at::Tensor decode_mla_plan(const at::Tensor &kv_seq_lens, int64_t num_kv_heads)
{
    const c10::DeviceGuard device_guard(kv_seq_lens.device());
    TORCH_CHECK(kv_seq_lens.scalar_type() == at::kInt && kv_seq_lens.is_contiguous() && kv_seq_lens.dim() == 1, "decode_mla_plan: kv_seq_lens must be int32 [batch]");
    const int B = (int)kv_seq_lens.size(0);
    const size_t bytes = mi_mla_decode_plan_bytes(B, (int)num_kv_heads);
    at::Tensor plan = at::empty({(int64_t)std::max<size_t>(bytes / 4, 4)}, at::dtype(at::kInt).device(kv_seq_lens.device()));
    if (B > 0)
        TORCH_CHECK(0 == mi_mla_decode_build_plan(kv_seq_lens.data_ptr<int>(), B, (int)num_kv_heads, plan.data_ptr(), bytes, cur_stream()),
                    "mi_mla_decode_build_plan failed");
    return plan;
}
void decode_mla_planned(const at::Tensor &q, const at::Tensor &k_nope_buffer, const at::Tensor &k_rope_buffer, at::Tensor &att_out,
                        const at::Tensor &kv_seq_lens, double sm_scale, int64_t page_size, const at::Tensor &block_table, const at::Tensor &plan)
{
    const c10::DeviceGuard device_guard(q.device());
    TORCH_CHECK(q.dim() == 3 && k_nope_buffer.dim() == 4 && k_rope_buffer.dim() == 4 && att_out.dim() == 3 && block_table.dim() == 2, "decode_mla: bad ranks");
    const int B = (int)q.size(0), Hq = (int)q.size(1), Hkv = (int)k_nope_buffer.size(2);
    // exact size: the list's item offsets depend on batch * kv heads (the size is strictly increasing in it), so a list built for a larger
    // batch must be refused, not read with the wrong offsets
    TORCH_CHECK(plan.scalar_type() == at::kInt && plan.is_contiguous() &&
                    (size_t)plan.numel() * 4 == std::max<size_t>(mi_mla_decode_plan_bytes(B, Hkv), 16),
                "decode_mla_planned: plan does not belong to this batch / kv head count");
    TORCH_CHECK(kv_seq_lens.dim() == 1 && kv_seq_lens.size(0) == B, "decode_mla_planned: kv_seq_lens must be [q.size(0)]");
    const bool shapes_ok = k_nope_buffer.size(3) == 512 && k_rope_buffer.size(3) == 64 && q.size(2) == 576 && att_out.size(2) == 512 &&
                           q.stride(2) == 1 && k_nope_buffer.stride(3) == 1 && k_rope_buffer.stride(3) == 1 && att_out.stride(2) == 1 &&
                           k_nope_buffer.size(1) == page_size && k_rope_buffer.size(1) == page_size && kv_seq_lens.scalar_type() == at::kInt &&
                           block_table.scalar_type() == at::kInt && kv_seq_lens.is_contiguous() && block_table.stride(1) == 1 && Hq % Hkv == 0;
    if (shapes_ok && B > 0) {
        const int max_len = (int)std::min<int64_t>(block_table.size(1) * page_size, INT32_MAX);
        const size_t wsb = mi_mla_decode_workspace(B, Hq, MI_MLA_SPLITS_PLANNED);
        at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(q.device()));
        const int rc = mi_mla_decode_with_plan(q.data_ptr(), k_nope_buffer.data_ptr(), k_rope_buffer.data_ptr(), att_out.data_ptr(),
                                               kv_seq_lens.data_ptr<int>(), block_table.data_ptr<int>(), B, Hq, Hkv, (int)page_size,
                                               (int)block_table.stride(0), max_len, q.stride(0), q.stride(1), k_nope_buffer.stride(0),
                                               k_nope_buffer.stride(1), k_nope_buffer.stride(2), k_rope_buffer.stride(0), k_rope_buffer.stride(1),
                                               k_rope_buffer.stride(2), att_out.stride(0), att_out.stride(1), (float)sm_scale, dtype_code(q),
                                               plan.data_ptr(), ws.data_ptr(), wsb, cur_stream());
        if (rc == 0) return;
        TORCH_CHECK(rc == MI_SGL_ENOTAPPLICABLE, "mi_mla_decode_with_plan failed with code ", rc);
    }
    // all checks live there; -1: the planned form with a list of its own where it applies, uniform splits where it does not (never back here)
    decode_mla(q, k_nope_buffer, k_rope_buffer, att_out, kv_seq_lens, sm_scale, page_size, block_table, MI_MLA_SPLITS_PLANNED);
}

// Paged GQA decode with a separate V cache; argument meaning of decode_gqa (decode_attention.py:378-387); writes att_out in place.
// A DeepSeek-style cache where V is the first 512 columns of the 576-wide K rows (the reference special-cases Lk == 576,
// :404-407, and its test builds exactly that view, test_decode_attention.py:74) goes to the MLA kernel, which reads each K
// row once for both GEMMs; everything else runs the generic kernel (csrc/kernels/gqa_decode.hip).
void decode_gqa(const at::Tensor &q, const at::Tensor &k_buffer, const at::Tensor &v_buffer, at::Tensor &att_out,
                const at::Tensor &kv_seq_lens, double sm_scale, int64_t page_size, const at::Tensor &block_table, int64_t num_splits)
{
    const c10::DeviceGuard device_guard(q.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(q.dim() == 3 && k_buffer.dim() == 4 && v_buffer.dim() == 4 && att_out.dim() == 3 && block_table.dim() == 2,
                "decode_gqa: bad ranks");
    TORCH_CHECK(q.stride(2) == 1 && k_buffer.stride(3) == 1 && v_buffer.stride(3) == 1 && att_out.stride(2) == 1,
                "decode_gqa: innermost dimension must be contiguous");
    TORCH_CHECK(k_buffer.size(1) == page_size && v_buffer.size(1) == page_size, "decode_gqa: page_size mismatch");
    TORCH_CHECK(q.scalar_type() == k_buffer.scalar_type() && q.scalar_type() == v_buffer.scalar_type() &&
                    q.scalar_type() == att_out.scalar_type(), "decode_gqa: dtype mismatch");
    TORCH_CHECK(kv_seq_lens.scalar_type() == at::kInt && block_table.scalar_type() == at::kInt && kv_seq_lens.is_contiguous(),
                "decode_gqa: kv_seq_lens / block_table must be int32");
    TORCH_CHECK(block_table.stride(1) == 1, "decode_gqa: block_table rows must be contiguous");
    const int B = (int)q.size(0), Hq = (int)q.size(1), Hkv = (int)k_buffer.size(2);
    const int Lk = (int)k_buffer.size(3), Lv = (int)v_buffer.size(3);
    TORCH_CHECK(Hq % Hkv == 0, "head_num must be divisible by kv_head_num");
    TORCH_CHECK(v_buffer.size(2) == Hkv && q.size(2) == Lk && att_out.size(2) == Lv && att_out.size(0) == B && att_out.size(1) == Hq,
                "decode_gqa: shape mismatch");
    const int max_len = (int)std::min<int64_t>(block_table.size(1) * page_size, INT32_MAX);   // upper bound, no host sync
    int splits = (int)num_splits;
    const bool v_is_k_prefix = Lk == 576 && Lv == 512 && v_buffer.data_ptr() == k_buffer.data_ptr() &&
                               v_buffer.stride(0) == k_buffer.stride(0) && v_buffer.stride(1) == k_buffer.stride(1) &&
                               v_buffer.stride(2) == k_buffer.stride(2);
    if (v_is_k_prefix && splits == 0 && k_buffer.size(1) == page_size) {
        // the library's choice: exactly decode_mla on the two column ranges of the K rows (the layers of a step then share its work list too)
        decode_mla(q, k_buffer.narrow(3, 0, 512), k_buffer.narrow(3, 512, 64), att_out, kv_seq_lens, sm_scale, page_size, block_table, 0);
        return;
    }
    if (v_is_k_prefix) {
        if (splits == 0) splits = mi_mla_decode_num_splits(B, Hq, Hkv, max_len);
        const size_t wsb = mi_mla_decode_workspace(B, Hq, splits);
        at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(q.device()));
        const char *kb = (const char *)k_buffer.data_ptr();
        const int rc = mi_mla_decode(q.data_ptr(), kb, kb + 512 * 2, att_out.data_ptr(), kv_seq_lens.data_ptr<int>(),
                                     block_table.data_ptr<int>(), B, Hq, Hkv, (int)page_size, (int)block_table.stride(0), max_len,
                                     q.stride(0), q.stride(1), k_buffer.stride(0), k_buffer.stride(1), k_buffer.stride(2),
                                     k_buffer.stride(0), k_buffer.stride(1), k_buffer.stride(2), att_out.stride(0),
                                     att_out.stride(1), (float)sm_scale, dtype_code(q), splits, ws.data_ptr(), wsb, cur_stream());
        TORCH_CHECK(rc == 0, "mi_mla_decode failed with code ", rc);
        return;
    }
    if (splits == 0) splits = mi_gqa_decode_num_splits(B, Hq, Hkv, max_len);
    const size_t wsb = mi_gqa_decode_workspace(B, Hq, Lv, splits);
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(q.device()));
    const int rc = mi_gqa_decode(q.data_ptr(), k_buffer.data_ptr(), v_buffer.data_ptr(), att_out.data_ptr(), kv_seq_lens.data_ptr<int>(),
                                 block_table.data_ptr<int>(), B, Hq, Hkv, Lk, Lv, (int)page_size, (int)block_table.stride(0), max_len,
                                 q.stride(0), q.stride(1), k_buffer.stride(0), k_buffer.stride(1), k_buffer.stride(2),
                                 v_buffer.stride(0), v_buffer.stride(1), v_buffer.stride(2), att_out.stride(0), att_out.stride(1),
                                 (float)sm_scale, dtype_code(q), splits, ws.data_ptr(), wsb, cur_stream());
    TORCH_CHECK(rc == 0, "mi_gqa_decode failed with code ", rc,
                " (head dims must be multiples of 8 with (k, v) <= (64,64) (128,128) (192,128) (256,256) (288,256) or (576,512))");
}

// attention/sinks_attention.py:90-137 (decode) and :241-286 (extend): query [rows, Hq * D]; kv_lens [rows] int32 = keys each query row sees;
// bt_rows [rows] int32 = its block-table row (undefined tensor = row index).  Returns [rows, Hq * Dv].
at::Tensor attention_sinks(const at::Tensor &query, const at::Tensor &k_cache, const at::Tensor &v_cache, const at::Tensor &sinks,
                           const at::Tensor &block_tables, const at::Tensor &kv_lens, double scale, int64_t sliding_window_size, int64_t q_head_num,
                           int64_t k_head_num, const std::optional<at::Tensor> &bt_rows)
{
    const c10::DeviceGuard device_guard(query.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(query.dim() == 2 && query.is_contiguous() && k_cache.dim() == 4 && v_cache.dim() == 4 && block_tables.dim() == 2,
                "attention_sinks: query [rows, Hq * D], caches [blocks, page, Hkv, D], block_tables [seqs, max_blocks]");
    TORCH_CHECK(k_cache.stride(3) == 1 && v_cache.stride(3) == 1 && block_tables.stride(1) == 1, "attention_sinks: innermost dimensions must be contiguous");
    TORCH_CHECK(query.scalar_type() == k_cache.scalar_type() && query.scalar_type() == v_cache.scalar_type(), "attention_sinks: dtype mismatch");
    TORCH_CHECK(kv_lens.scalar_type() == at::kInt && kv_lens.is_contiguous() && block_tables.scalar_type() == at::kInt,
                "attention_sinks: kv lengths / block_tables must be int32");
    const int rows = (int)query.size(0), Hq = (int)q_head_num, Hkv = (int)k_head_num;
    TORCH_CHECK(Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && query.size(1) % Hq == 0 && k_cache.size(2) == Hkv && v_cache.size(2) == Hkv, "attention_sinks: heads");
    const int D = (int)(query.size(1) / Hq), Dv = (int)v_cache.size(3);
    TORCH_CHECK(k_cache.size(3) == D && kv_lens.numel() == rows, "attention_sinks: shape mismatch");
    TORCH_CHECK(sinks.numel() == Hq && sinks.is_contiguous(), "attention_sinks: sinks must hold one value per q head");
    if (bt_rows.has_value()) TORCH_CHECK(bt_rows->scalar_type() == at::kInt && bt_rows->is_contiguous() && bt_rows->numel() == rows, "attention_sinks: bt_rows");
    const int page = (int)k_cache.size(1);
    at::Tensor out = at::empty({rows, (int64_t)Hq * Dv}, query.options());
    int64_t max_len = std::min<int64_t>(block_tables.size(1) * (int64_t)page, INT32_MAX);
    if (sliding_window_size >= 0) max_len = std::min<int64_t>(max_len, std::max<int64_t>(sliding_window_size, 1));
    const int splits = mi_gqa_decode_num_splits(rows, Hq, Hkv, (int)max_len);
    const size_t wsb = mi_gqa_decode_workspace(rows, Hq, Dv, splits);
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(query.device()));
    const int rc = mi_gqa_decode_sinks(query.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), kv_lens.data_ptr<int>(),
                                       block_tables.data_ptr<int>(), rows, Hq, Hkv, D, Dv, page, (int)block_tables.stride(0), (int)max_len,
                                       (int64_t)Hq * D, D, k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), v_cache.stride(0),
                                       v_cache.stride(1), v_cache.stride(2), (int64_t)Hq * Dv, Dv, (float)scale, dtype_code(query), splits,
                                       ws.data_ptr(), wsb, sinks.data_ptr(), dtype_code3(sinks), (int)sliding_window_size,
                                       bt_rows.has_value() ? bt_rows->data_ptr<int>() : nullptr, cur_stream());
    TORCH_CHECK(rc == 0, "mi_gqa_decode_sinks failed with code ", rc);
    return out;
}

// attention/fia_blockq_attention.py:89-181: per-query block tables (mi_fia_prep), then a paged decode with one query row per "sequence"
at::Tensor fia_blockq_sparse_prefill(const at::Tensor &q, const at::Tensor &k_cache, const at::Tensor &v_cache, const at::Tensor &topk_idx,
                                     const at::Tensor &seq_lens, const at::Tensor &per_query_req, const at::Tensor &req_to_token,
                                     int64_t block_size, double sm_scale, const std::optional<at::Tensor> &block_table_out,
                                     const std::optional<at::Tensor> &actual_kvlen_out)
{
    const c10::DeviceGuard device_guard(q.device());
    TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4 && topk_idx.dim() == 2 && req_to_token.dim() == 2, "fia_blockq_sparse_prefill: bad ranks");
    TORCH_CHECK(topk_idx.scalar_type() == at::kInt && seq_lens.scalar_type() == at::kInt && req_to_token.scalar_type() == at::kInt,
                "fia_blockq_sparse_prefill: topk_idx / seq_lens / req_to_token must be int32");
    TORCH_CHECK(per_query_req.scalar_type() == at::kInt || per_query_req.scalar_type() == at::kLong, "per_query_req must be int32 or int64");
    const int64_t total_q = q.size(0), topk1 = topk_idx.size(1);
    TORCH_CHECK(topk_idx.size(0) == total_q && seq_lens.numel() == total_q && per_query_req.numel() == total_q && seq_lens.is_contiguous() &&
                    per_query_req.is_contiguous() && topk1 <= 64 && k_cache.size(1) == block_size,
                "fia_blockq_sparse_prefill: shape mismatch (topk + 1 <= 64)");
    at::Tensor bt = block_table_out.has_value() ? *block_table_out : at::empty({total_q, topk1}, topk_idx.options());
    at::Tensor kvl = actual_kvlen_out.has_value() ? *actual_kvlen_out : at::empty({total_q}, topk_idx.options());
    TORCH_CHECK(bt.scalar_type() == at::kInt && bt.dim() == 2 && bt.size(0) == total_q && bt.size(1) == topk1 && bt.stride(1) == 1 &&
                    kvl.scalar_type() == at::kInt && kvl.numel() == total_q && kvl.is_contiguous(), "block_table_out / actual_kvlen_out");
    const int rc = mi_fia_prep(topk_idx.data_ptr<int>(), topk_idx.stride(0), topk_idx.stride(1), seq_lens.data_ptr<int>(), per_query_req.data_ptr(),
                               per_query_req.scalar_type() == at::kLong, req_to_token.data_ptr<int>(), req_to_token.stride(0),
                               req_to_token.stride(1), (int)req_to_token.size(1), (int)total_q, (int)topk1, (int)block_size, bt.data_ptr<int>(),
                               bt.stride(0), kvl.data_ptr<int>(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_fia_prep failed with code ", rc);
    at::Tensor out = at::empty({total_q, q.size(1), v_cache.size(3)}, q.options());
    if (total_q > 0) decode_gqa(q, k_cache, v_cache, out, kvl, sm_scale, block_size, bt, 0);
    return out;
}

// attention/gqa_share_sparse_attention.py:635-878: block-sparse GQA decode over the top-k selected KV blocks (csrc/kernels/gqa_sparse_decode.hip).
// topk_idx [Hkv or Hq, B, topk] (per-q-head lists: the list of each group's first head is used, :734-739); exactly one of block_table and
// (req_to_token, req_pool_indices, max_num_blocks, num_pages); num_chunks 0 = the library's choice.  Returns [B, Hq, D].
at::Tensor gqa_share_sparse_decode(const at::Tensor &q, const std::optional<at::Tensor> &sink, const at::Tensor &k_cache, const at::Tensor &v_cache,
                                   const std::optional<at::Tensor> &block_table, const at::Tensor &seq_lens, const at::Tensor &topk_idx,
                                   double sm_scale, int64_t num_chunks, const std::optional<at::Tensor> &req_to_token,
                                   const std::optional<at::Tensor> &req_pool_indices, int64_t max_num_blocks, int64_t num_pages,
                                   bool sanitize_page_ids)
{
    const c10::DeviceGuard device_guard(q.device());
    auto is_index = [](const at::Tensor &t) { return t.scalar_type() == at::kInt || t.scalar_type() == at::kLong; };
    TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4 && v_cache.dim() == 4 && topk_idx.dim() == 3 && seq_lens.dim() == 1,
                "gqa_share_sparse_decode: q [B, Hq, D], caches [pages, block, Hkv, D], topk_idx [H, B, topk], seq_lens [B]");
    TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "gqa_share_sparse_decode: q must be fp16 or bf16");
    TORCH_CHECK(k_cache.scalar_type() == q.scalar_type() && v_cache.scalar_type() == q.scalar_type(), "gqa_share_sparse_decode: dtype mismatch");
    TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), "gqa_share_sparse_decode: k / v cache shapes differ");
    TORCH_CHECK(q.stride(2) == 1 && k_cache.stride(3) == 1 && v_cache.stride(3) == 1, "gqa_share_sparse_decode: innermost dimension must be contiguous");
    const int64_t B = q.size(0), Hq = q.size(1), D = q.size(2), block_size = k_cache.size(1), Hkv = k_cache.size(2), topk = topk_idx.size(2);
    TORCH_CHECK(k_cache.size(3) == D && Hkv > 0 && Hq % Hkv == 0 && seq_lens.size(0) == B && topk_idx.size(1) == B,
                "gqa_share_sparse_decode: shape mismatch");
    TORCH_CHECK(topk_idx.size(0) == Hkv || topk_idx.size(0) == Hq, "gqa_share_sparse_decode: topk_idx must hold one list per kv head or per q head");
    TORCH_CHECK(is_index(topk_idx) || topk_idx.scalar_type() == at::kShort || topk_idx.scalar_type() == at::kChar || topk_idx.scalar_type() == at::kByte,
                "gqa_share_sparse_decode: topk_idx must be an integer tensor");
    TORCH_CHECK(is_index(seq_lens), "gqa_share_sparse_decode: seq_lens must be int32 or int64");
    const bool direct = req_to_token.has_value();
    TORCH_CHECK(direct == req_pool_indices.has_value() && direct != block_table.has_value(),
                "gqa_share_sparse_decode: exactly one of block_table and (req_to_token, req_pool_indices)");
    int64_t max_kv_len;
    if (direct) {
        TORCH_CHECK(req_to_token->dim() == 2 && is_index(*req_to_token) && req_pool_indices->dim() == 1 && is_index(*req_pool_indices) &&
                        req_pool_indices->size(0) == B && req_pool_indices->is_contiguous(), "gqa_share_sparse_decode: req_to_token / req_pool_indices");
        TORCH_CHECK(max_num_blocks > 0 && num_pages > 0 && max_num_blocks * block_size <= req_to_token->size(1),
                    "gqa_share_sparse_decode: max_num_blocks / num_pages");
        max_kv_len = max_num_blocks * block_size;
    } else {
        TORCH_CHECK(block_table->dim() == 2 && is_index(*block_table) && block_table->size(0) == B, "gqa_share_sparse_decode: block_table");
        max_kv_len = block_table->size(1) * block_size;
    }
    max_kv_len = std::min<int64_t>(max_kv_len, INT32_MAX);
    const at::Tensor lens = seq_lens.scalar_type() == at::kInt && seq_lens.is_contiguous() ? seq_lens : seq_lens.to(at::kInt).contiguous();
    const at::Tensor idx = (is_index(topk_idx)) ? topk_idx : topk_idx.to(at::kInt);
    const int64_t idx_sh = idx.stride(0) * (idx.size(0) == Hkv ? 1 : Hq / Hkv);
    at::Tensor sk;
    if (sink.has_value()) {
        TORCH_CHECK(sink->dim() == 2 && sink->size(0) == Hq && sink->size(1) == D, "gqa_share_sparse_decode: sink must be [Hq, D]");
        sk = sink->scalar_type() == at::kFloat || sink->scalar_type() == q.scalar_type() ? *sink : sink->to(at::kFloat);
        if (sk.stride(1) != 1) sk = sk.contiguous();
    }
    TORCH_CHECK(num_chunks >= 0, "gqa_share_sparse_decode: num_chunks");
    int chunks = (int)num_chunks;
    if (chunks == 0) chunks = mi_gqa_sparse_decode_num_chunks((int)B, (int)Hkv, (int)topk);
    at::Tensor out = at::empty({B, Hq, D}, q.options());
    const size_t wsb = mi_gqa_sparse_decode_workspace((int)B, (int)Hq, (int)D, chunks);
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(q.device()));
    const at::Tensor *tab = direct ? &*req_to_token : &*block_table;
    const int rc = mi_gqa_sparse_decode(
        q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), lens.data_ptr<int>(), idx.data_ptr(), idx.scalar_type() == at::kLong,
        idx_sh, idx.stride(1), idx.stride(2), direct ? nullptr : tab->data_ptr(), tab->scalar_type() == at::kLong, tab->stride(0), tab->stride(1),
        direct ? tab->data_ptr() : nullptr, tab->scalar_type() == at::kLong, tab->stride(0), tab->stride(1), direct ? (int)tab->size(1) : 0,
        direct ? req_pool_indices->data_ptr() : nullptr, direct && req_pool_indices->scalar_type() == at::kLong,
        sk.defined() ? sk.data_ptr() : nullptr, sk.defined() ? dtype_code3(sk) : 0, sk.defined() ? sk.stride(0) : 0, (int)B, (int)Hq, (int)Hkv, (int)D,
        (int)block_size, (int)topk, (int)max_kv_len, direct ? (int)num_pages : 1, sanitize_page_ids, q.stride(0), q.stride(1), k_cache.stride(0),
        k_cache.stride(1), k_cache.stride(2), v_cache.stride(0), v_cache.stride(1), v_cache.stride(2), out.stride(0), out.stride(1), (float)sm_scale,
        dtype_code(q), chunks, ws.data_ptr(), wsb, cur_stream());
    TORCH_CHECK(rc == 0, "mi_gqa_sparse_decode failed with code ", rc,
                " (head_dim a multiple of 8 up to 256, block_size 16 / 32 / 64 / 128, 1 <= num_chunks <= max(1, topk), at most 1024 list slots per chunk)");
    return out;
}

// the chunk count gqa_share_sparse_decode picks for num_chunks = 0 (host arithmetic; a power of two)
int64_t gqa_share_sparse_num_chunks(int64_t batch, int64_t kv_heads, int64_t topk)
{
    return mi_gqa_sparse_decode_num_chunks((int)batch, (int)kv_heads, (int)std::min<int64_t>(topk, INT32_MAX));
}

// indexer/flash_block_score_decode.py:1571-1889, score-only form: block scores + top-k selection (csrc/kernels/gqa_block_score.hip).
// Returns topk_idx [Hq, B, topk] int32, or [Hq, B, topk + 1] with append_local (max_num_blocks > 0 then: the causal-local block's bound).
// seq_lens [B], or [B * group] with packed_seq_lens; exactly one of block_table and (req_to_token, req_pool_indices, num_pages).
at::Tensor gqa_block_score_topk(const at::Tensor &q, const at::Tensor &k_cache, const std::optional<at::Tensor> &block_table,
                                const at::Tensor &seq_lens, int64_t max_seqlen, int64_t topk, int64_t init_blocks, int64_t local_blocks,
                                double sm_scale, bool score_lse, const std::optional<at::Tensor> &req_to_token,
                                const std::optional<at::Tensor> &req_pool_indices, int64_t max_num_blocks, int64_t num_pages,
                                bool sanitize_page_ids, bool packed_seq_lens, bool append_local)
{
    const c10::DeviceGuard device_guard(q.device());
    auto is_index = [](const at::Tensor &t) { return t.scalar_type() == at::kInt || t.scalar_type() == at::kLong; };
    TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4 && seq_lens.dim() == 1, "gqa_block_score_topk: q [B, Hq, D], k_cache [pages, block, Hkv, D], seq_lens 1-d");
    TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "gqa_block_score_topk: q must be fp16 or bf16");
    TORCH_CHECK(k_cache.scalar_type() == q.scalar_type(), "gqa_block_score_topk: dtype mismatch");
    TORCH_CHECK(q.stride(2) == 1 && k_cache.stride(3) == 1, "gqa_block_score_topk: innermost dimension must be contiguous");
    const int64_t B = q.size(0), Hq = q.size(1), D = q.size(2), block_size = k_cache.size(1), Hkv = k_cache.size(2);
    TORCH_CHECK(k_cache.size(3) == D && Hkv > 0 && Hq % Hkv == 0, "gqa_block_score_topk: shape mismatch");
    TORCH_CHECK(is_index(seq_lens) && seq_lens.size(0) == (packed_seq_lens ? B * (Hq / Hkv) : B), "gqa_block_score_topk: seq_lens");
    const bool direct = req_to_token.has_value();
    TORCH_CHECK(direct == req_pool_indices.has_value() && direct != block_table.has_value(),
                "gqa_block_score_topk: exactly one of block_table and (req_to_token, req_pool_indices)");
    if (direct) {
        TORCH_CHECK(req_to_token->dim() == 2 && is_index(*req_to_token) && req_pool_indices->dim() == 1 && is_index(*req_pool_indices) &&
                        req_pool_indices->size(0) == B && req_pool_indices->is_contiguous(), "gqa_block_score_topk: req_to_token / req_pool_indices");
        TORCH_CHECK(num_pages > 0, "gqa_block_score_topk: num_pages");
    } else {
        TORCH_CHECK(block_table->dim() == 2 && is_index(*block_table) && block_table->size(0) == B && block_table->size(1) > 0,
                    "gqa_block_score_topk: block_table");
    }
    TORCH_CHECK(block_size > 0 && max_seqlen > 0, "gqa_block_score_topk: max_seqlen");
    const int64_t max_seqblock = (max_seqlen + block_size - 1) / block_size;
    TORCH_CHECK(max_seqblock <= 16384, "gqa_block_score_topk: max_seqlen spans ", max_seqblock, " blocks, the limit is 16384");
    TORCH_CHECK(topk >= 1 && topk <= 1024, "gqa_block_score_topk: topk must lie in [1, 1024]");
    TORCH_CHECK(init_blocks >= 0 && local_blocks >= 0 && init_blocks <= INT32_MAX && local_blocks <= INT32_MAX, "gqa_block_score_topk: init / local blocks");
    TORCH_CHECK(!append_local || (max_num_blocks > 0 && max_num_blocks <= INT32_MAX), "gqa_block_score_topk: append_local needs max_num_blocks");
    const at::Tensor lens = seq_lens.scalar_type() == at::kInt && seq_lens.is_contiguous() ? seq_lens : seq_lens.to(at::kInt).contiguous();
    at::Tensor out = at::empty({Hq, B, topk + (append_local ? 1 : 0)}, q.options().dtype(at::kInt));
    const size_t wsb = mi_gqa_block_score_topk_workspace((int)B, (int)Hq, (int)max_seqblock);
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(q.device()));
    const at::Tensor *tab = direct ? &*req_to_token : &*block_table;
    const int rc = mi_gqa_block_score_topk(
        q.data_ptr(), k_cache.data_ptr(), out.data_ptr<int>(), lens.data_ptr<int>(), packed_seq_lens, direct ? nullptr : tab->data_ptr(),
        tab->scalar_type() == at::kLong, tab->stride(0), tab->stride(1), direct ? 0 : (int)std::min<int64_t>(tab->size(1), INT32_MAX),
        direct ? tab->data_ptr() : nullptr, tab->scalar_type() == at::kLong, tab->stride(0), tab->stride(1),
        direct ? (int)std::min<int64_t>(tab->size(1), INT32_MAX) : 0, direct ? req_pool_indices->data_ptr() : nullptr,
        direct && req_pool_indices->scalar_type() == at::kLong, (int)B, (int)Hq, (int)Hkv, (int)D, (int)block_size, (int)max_seqblock, (int)topk,
        (int)init_blocks, (int)local_blocks, score_lse, append_local ? (int)max_num_blocks : 0, direct ? (int)num_pages : 1, sanitize_page_ids,
        q.stride(0), q.stride(1), k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), (float)sm_scale, dtype_code(q), ws.data_ptr(), wsb,
        cur_stream());
    TORCH_CHECK(rc == 0, "mi_gqa_block_score_topk failed with code ", rc,
                " (head_dim a multiple of 8 up to 256, block_size 16 / 32 / 64 / 128, sm_scale > 0, strides multiples of 8 elements)");
    return out;
}

// indexer/flash_block_score_decode.py:1519-1562: [H, B, topk] int32 -> [H, B, topk + 1] with the causal-local block appended
at::Tensor topk_append_local_block(const at::Tensor &topk_idx, const at::Tensor &seq_lens, int64_t block_size, int64_t num_blocks)
{
    const c10::DeviceGuard device_guard(topk_idx.device());
    TORCH_CHECK(topk_idx.dim() == 3 && topk_idx.scalar_type() == at::kInt && topk_idx.is_contiguous(), "topk_append_local_block: topk_idx [H, B, topk] int32, contiguous");
    TORCH_CHECK(seq_lens.dim() == 1 && seq_lens.size(0) == topk_idx.size(1) && (seq_lens.scalar_type() == at::kInt || seq_lens.scalar_type() == at::kLong),
                "topk_append_local_block: seq_lens [B], int32 or int64");
    TORCH_CHECK(block_size > 0 && block_size <= INT32_MAX && num_blocks > 0 && num_blocks <= INT32_MAX, "topk_append_local_block: block_size / num_blocks");
    const at::Tensor lens = seq_lens.scalar_type() == at::kInt && seq_lens.is_contiguous() ? seq_lens : seq_lens.to(at::kInt).contiguous();
    at::Tensor out = at::empty({topk_idx.size(0), topk_idx.size(1), topk_idx.size(2) + 1}, topk_idx.options());
    const int rc = mi_topk_append_local_block(topk_idx.data_ptr<int>(), lens.data_ptr<int>(), out.data_ptr<int>(), (int)topk_idx.size(0),
                                              (int)topk_idx.size(1), (int)topk_idx.size(2), (int)block_size, (int)num_blocks, cur_stream());
    TORCH_CHECK(rc == 0, "mi_topk_append_local_block failed with code ", rc);
    return out;
}

// indexer/flash_block_score_prefill.py:434-557: block scores of every query token of a prefill chunk (csrc/kernels/gqa_block_score_prefill.hip).
// Returns score [Hidx, total_q, ceil(max_seqlen / block)] fp32, every element written.  query_pos [total_q]: the position each token's causal
// mask compares with; absent = the token's true position seq_lens[r] - q_len[r] + i.
at::Tensor gqa_prefill_block_score(const at::Tensor &q, const at::Tensor &k_cache, const at::Tensor &cu_seqlens, const at::Tensor &seq_lens,
                                   const at::Tensor &req_to_token, const at::Tensor &req_pool_indices, int64_t max_seqlen, double sm_scale,
                                   bool score_lse, const std::optional<at::Tensor> &query_pos)
{
    const c10::DeviceGuard device_guard(q.device());
    auto is_index = [](const at::Tensor &t) { return t.scalar_type() == at::kInt || t.scalar_type() == at::kLong; };
    TORCH_CHECK(q.dim() == 3 && k_cache.dim() == 4, "gqa_prefill_block_score: q [total_q, Hidx, D], k_cache [pages, block, Hkv, D]");
    TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "gqa_prefill_block_score: q must be fp16 or bf16");
    TORCH_CHECK(k_cache.scalar_type() == q.scalar_type(), "gqa_prefill_block_score: dtype mismatch");
    TORCH_CHECK(q.stride(2) == 1 && k_cache.stride(3) == 1, "gqa_prefill_block_score: innermost dimension must be contiguous");
    const int64_t total_q = q.size(0), Hidx = q.size(1), D = q.size(2), block_size = k_cache.size(1), Hkv = k_cache.size(2);
    TORCH_CHECK(k_cache.size(3) == D && Hkv > 0 && Hidx > 0 && Hidx % Hkv == 0, "gqa_prefill_block_score: shape mismatch");
    TORCH_CHECK(total_q <= INT32_MAX, "gqa_prefill_block_score: total_q");
    TORCH_CHECK(cu_seqlens.dim() == 1 && is_index(cu_seqlens) && cu_seqlens.size(0) >= 1 && cu_seqlens.is_contiguous(), "gqa_prefill_block_score: cu_seqlens");
    const int64_t n = cu_seqlens.size(0) - 1;
    TORCH_CHECK(seq_lens.dim() == 1 && is_index(seq_lens) && seq_lens.size(0) == n && seq_lens.is_contiguous(), "gqa_prefill_block_score: seq_lens [n]");
    TORCH_CHECK(req_pool_indices.dim() == 1 && is_index(req_pool_indices) && req_pool_indices.size(0) == n && req_pool_indices.is_contiguous(),
                "gqa_prefill_block_score: req_pool_indices [n]");
    TORCH_CHECK(req_to_token.dim() == 2 && is_index(req_to_token) && req_to_token.size(1) > 0, "gqa_prefill_block_score: req_to_token [requests, columns]");
    if (query_pos.has_value())
        TORCH_CHECK(query_pos->dim() == 1 && is_index(*query_pos) && query_pos->size(0) == total_q && query_pos->is_contiguous(),
                    "gqa_prefill_block_score: query_pos [total_q]");
    TORCH_CHECK(block_size > 0 && max_seqlen > 0, "gqa_prefill_block_score: max_seqlen");
    const int64_t max_seqblock = (max_seqlen + block_size - 1) / block_size;
    TORCH_CHECK(max_seqblock <= 16384, "gqa_prefill_block_score: max_seqlen spans ", max_seqblock, " blocks, the limit is 16384");
    at::Tensor score = at::empty({Hidx, total_q, max_seqblock}, q.options().dtype(at::kFloat));
    const int rc = mi_gqa_prefill_block_score(
        q.data_ptr(), k_cache.data_ptr(), score.data_ptr<float>(), cu_seqlens.data_ptr(), cu_seqlens.scalar_type() == at::kLong, seq_lens.data_ptr(),
        seq_lens.scalar_type() == at::kLong, req_to_token.data_ptr(), req_to_token.scalar_type() == at::kLong, req_to_token.stride(0),
        req_to_token.stride(1), (int)std::min<int64_t>(req_to_token.size(1), INT32_MAX), req_pool_indices.data_ptr(),
        req_pool_indices.scalar_type() == at::kLong, query_pos.has_value() ? query_pos->data_ptr() : nullptr,
        query_pos.has_value() && query_pos->scalar_type() == at::kLong, (int)total_q, (int)n, (int)Hidx, (int)Hkv, (int)D, (int)block_size,
        (int)max_seqblock, score_lse, q.stride(0), q.stride(1), k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), score.stride(0),
        score.stride(1), (float)sm_scale, dtype_code(q), cur_stream());
    TORCH_CHECK(rc == 0, "mi_gqa_prefill_block_score failed with code ", rc,
                " (head_dim a multiple of 8 up to 256, block_size 16 / 32 / 64 / 128, sm_scale > 0, strides multiples of 8 elements)");
    return score;
}

// indexer/flash_block_score_prefill.py:761-811 (fused) and the torch.topk branch of :895-909 (not fused): score [H, total_q, blocks] fp32 ->
// topk_idx [H, total_q, topk (+ 1 fused)] int32
at::Tensor prefill_topk_from_score(const at::Tensor &score, const std::optional<at::Tensor> &per_query_seq_lens, int64_t topk, int64_t block_size,
                                   bool fused)
{
    const c10::DeviceGuard device_guard(score.device());
    TORCH_CHECK(score.dim() == 3 && score.scalar_type() == at::kFloat, "prefill_topk_from_score: score [H, total_q, blocks] fp32");
    TORCH_CHECK(score.size(2) >= 1 && score.size(2) <= 16384, "prefill_topk_from_score: 1 .. 16384 blocks are served");
    TORCH_CHECK(topk >= 1 && topk <= 1024, "prefill_topk_from_score: topk must lie in [1, 1024]");
    TORCH_CHECK(block_size > 0 && block_size <= INT32_MAX && score.size(1) <= INT32_MAX && score.size(0) <= INT32_MAX, "prefill_topk_from_score: sizes");
    TORCH_CHECK(!fused || per_query_seq_lens.has_value(), "prefill_topk_from_score: the fused form needs per_query_seq_lens");
    const void *lens = nullptr;
    bool lens_i64 = false;
    if (fused) {
        const at::Tensor &l = *per_query_seq_lens;
        TORCH_CHECK(l.dim() == 1 && l.size(0) == score.size(1) && l.is_contiguous() && (l.scalar_type() == at::kInt || l.scalar_type() == at::kLong),
                    "prefill_topk_from_score: per_query_seq_lens [total_q], int32 or int64");
        lens = l.data_ptr(), lens_i64 = l.scalar_type() == at::kLong;
    }
    at::Tensor out = at::empty({score.size(0), score.size(1), topk + (fused ? 1 : 0)}, score.options().dtype(at::kInt));
    const int rc = mi_prefill_topk_from_score(score.data_ptr<float>(), score.stride(0), score.stride(1), score.stride(2), lens, lens_i64,
                                              out.data_ptr<int>(), (int)score.size(0), (int)score.size(1), (int)score.size(2), (int)topk,
                                              (int)block_size, fused, cur_stream());
    TORCH_CHECK(rc == 0, "mi_prefill_topk_from_score failed with code ", rc);
    return out;
}

// csrc/lightning_indexer/op_host/lightning_indexer.cpp:61-169 (checks: op_host/tiling/lightning_indexer_tiling.cpp:111-479, whose wording the
// messages keep): the token-level top-k indexer of DeepSeek-V3.2 (csrc/kernels/lightning_indexer.hip).  Defaults as the reference's op
// definition: layout_query "TND", layout_key "PA_BSND", sparse_count 2048, sparse_mode 3.  Returns sparse_indices int32,
// [B, S1, 1, sparse_count] (BSND) or [T, 1, sparse_count] (TND): the visible keys of highest score, descending, then -1.
at::Tensor lightning_indexer(const at::Tensor &query, const at::Tensor &key, const at::Tensor &weights,
                             const std::optional<at::Tensor> &actual_seq_lengths_query, const std::optional<at::Tensor> &actual_seq_lengths_key,
                             const std::optional<at::Tensor> &block_table, std::optional<c10::string_view> layout_query,
                             std::optional<c10::string_view> layout_key, std::optional<int64_t> sparse_count, std::optional<int64_t> sparse_mode)
{
    const c10::DeviceGuard device_guard(query.device());   // launches and the current stream follow the tensor's GPU
    const std::string lq(layout_query.value_or("TND")), lk(layout_key.value_or("PA_BSND"));
    const int64_t count = sparse_count.value_or(2048), mode = sparse_mode.value_or(3);
    TORCH_CHECK(lk == "PA_BSND" || lq == lk, "lightning_indexer: under non-PA conditions, layout_query and layout_key should be equal.");
    TORCH_CHECK(lk == "PA_BSND" || lk == "BSND" || lk == "TND", "lightning_indexer: input attr layout_key only supported PA_BSND, BSND or TND");
    TORCH_CHECK(lq == "BSND" || lq == "TND", "lightning_indexer: input attr layout_query only supported BSND or TND");
    TORCH_CHECK(count > 0 && count <= 2048, "lightning_indexer: input attr sparse_count must > 0 and <= 2048.");
    TORCH_CHECK(mode == 0 || mode == 3, "lightning_indexer: input attr sparse_mode only supported 0 or 3.");
    TORCH_CHECK(query.scalar_type() == key.scalar_type() && key.scalar_type() == weights.scalar_type(),
                "lightning_indexer: The data types of the input query, key, and weights must be the same.");
    TORCH_CHECK(query.scalar_type() == at::kHalf || query.scalar_type() == at::kBFloat16,
                "lightning_indexer: The data types of the input query, key, and weights must be float16 or bfloat16.");
    const bool q_tnd = lq == "TND", paged = lk == "PA_BSND", k_tnd = lk == "TND";
    auto int32_1d = [](const std::optional<at::Tensor> &t) { return !t.has_value() || t->scalar_type() == at::kInt; };
    if (paged) {
        TORCH_CHECK(block_table.has_value(), "lightning_indexer: key layout only supported PA_BSND, input block_table must not be null");
        TORCH_CHECK(actual_seq_lengths_key.has_value(),
                    "lightning_indexer: key layout only supported PA_BSND, input actual_seq_lengths_key must not be null");
        TORCH_CHECK(block_table->scalar_type() == at::kInt, "lightning_indexer: input block_table data type only support int32");
    } else {
        TORCH_CHECK(!k_tnd || actual_seq_lengths_key.has_value(),
                    "lightning_indexer: when layout_key is TND, input actual_seq_lengths_key must not be null");
        TORCH_CHECK(!block_table.has_value(), "lightning_indexer: when key layout is not PA_BSND, input block_table must be null");
    }
    TORCH_CHECK(int32_1d(actual_seq_lengths_key), "lightning_indexer: input actual_seq_lengths_key data type only support int32");
    TORCH_CHECK(!q_tnd || actual_seq_lengths_query.has_value(),
                "lightning_indexer: when layout_query is TND, input actual_seq_lengths_query must not be null");
    TORCH_CHECK(int32_1d(actual_seq_lengths_query), "lightning_indexer: input actual_seq_lengths_query data type only support int32");
    TORCH_CHECK(!block_table.has_value() || block_table->dim() == 2, "lightning_indexer: the dim num of block_table's shape should be 2");
    const int64_t qd = q_tnd ? 3 : 4, kd = k_tnd ? 3 : 4;
    TORCH_CHECK(key.dim() == kd, "lightning_indexer: the dim num of key's shape should be ", kd, ", but now is ", key.dim());
    TORCH_CHECK(query.dim() == qd, "lightning_indexer: the dim num of query's shape should be ", qd, ", but now is ", query.dim());
    TORCH_CHECK(weights.dim() == qd - 1, "lightning_indexer: the dim num of weights's shape should be ", qd - 1, ", but now is ", weights.dim());
    for (int64_t i = 0; i < query.dim(); ++i)
        TORCH_CHECK(query.size(i) > 0, "All values within query's shape should be greater than 0, but shape[", i, "] is ", query.size(i));
    const int64_t n1 = query.size(qd - 2), D = query.size(qd - 1), n2 = key.size(k_tnd ? 1 : 2);
    TORCH_CHECK(n2 == 1, "lightning_indexer: key shape", k_tnd ? 1 : 2, " is numhead, only support 1.");
    TORCH_CHECK(n1 / n2 == 64 && n1 % n2 == 0, "lightning_indexer: N1 is ", n1, ", N2 is ", n2, ", N1 divided by N2 must equal 64.");
    TORCH_CHECK(D == 128, "lightning_indexer: input query's last dim head_dim only support 128.");
    TORCH_CHECK(key.size(kd - 1) == D, "lightning_indexer: input query, key shape last dim must be same.");
    TORCH_CHECK(weights.size(qd - 2) == n1, "lightning_indexer: input query, weight shape dim N1 must be same.");
    const int64_t B = q_tnd ? actual_seq_lengths_query->numel() : query.size(0), S1 = q_tnd ? 1 : query.size(1);
    const int64_t rows = q_tnd ? query.size(0) : B * S1;
    TORCH_CHECK(B > 0 && B <= INT32_MAX && S1 <= INT32_MAX, "lightning_indexer: batch size");
    if (q_tnd) {
        TORCH_CHECK(weights.size(0) == rows, "lightning_indexer: TND case input query, weights dim 0 must be same.");
    } else {
        TORCH_CHECK(weights.size(0) == B && weights.size(1) == S1, "lightning_indexer: BSND case input query, weight dim 0 and dim 1 must be same.");
        TORCH_CHECK(!actual_seq_lengths_query.has_value() || actual_seq_lengths_query->numel() == B,
                    "lightning_indexer: BSND case input query, actual_seq_lengths_query dim 0 must be same");
    }
    TORCH_CHECK(!actual_seq_lengths_key.has_value() || actual_seq_lengths_key->numel() == B,
                "lightning_indexer: input actual_seq_lengths_query, actual_seq_lengths_key dim 0 must be same.");
    TORCH_CHECK(!block_table.has_value() || block_table->size(0) == B, "lightning_indexer: input block_table dim 0 must be the batch size.");
    int64_t block_size = 0, cap;
    if (paged) {
        block_size = key.size(1);
        TORCH_CHECK(block_size % 16 == 0 && block_size > 0 && block_size <= 1024,
                    "lightning_indexer: input key's block_size must be a multiple of 16 and belong to (0, 1024].");
        TORCH_CHECK(key.size(0) != 0, "lightning_indexer: input key's block_count cannot be 0.");
        TORCH_CHECK(block_table->size(1) > 0, "lightning_indexer: block_table needs at least one column");
        cap = block_table->size(1) * block_size;
    } else {
        cap = k_tnd ? key.size(0) : key.size(1);
        TORCH_CHECK(k_tnd || key.size(0) == B, "lightning_indexer: BSND case input query, key dim 0 must be same.");
    }
    TORCH_CHECK(cap >= 1 && cap <= MI_LIGHTNING_INDEXER_MAX_KEYS, "lightning_indexer: a sequence may hold up to ", MI_LIGHTNING_INDEXER_MAX_KEYS,
                " keys here (block_table columns * block_size, or the key's sequence dimension), but now it is ", cap);
    TORCH_CHECK(query.stride(qd - 1) == 1 && key.stride(kd - 1) == 1, "lightning_indexer: innermost dimension must be contiguous");
    auto i32c = [](const std::optional<at::Tensor> &t) { return t.has_value() ? std::optional<at::Tensor>(t->contiguous()) : std::nullopt; };
    const std::optional<at::Tensor> aq = i32c(actual_seq_lengths_query), ak = i32c(actual_seq_lengths_key);
    const std::optional<at::Tensor> bt = block_table.has_value() && block_table->stride(1) != 1 ? i32c(block_table) : block_table;
    const at::Tensor w = weights.stride(qd - 2) == 1 ? weights : weights.contiguous();
    std::vector<int64_t> shape = q_tnd ? std::vector<int64_t>{rows, n2, count} : std::vector<int64_t>{B, S1, n2, count};
    at::Tensor out = at::empty(shape, query.options().dtype(at::kInt));
    const int lqc = q_tnd ? MI_LI_QUERY_TND : MI_LI_QUERY_BSND, lkc = paged ? MI_LI_KEY_PA_BSND : k_tnd ? MI_LI_KEY_TND : MI_LI_KEY_BSND;
    const size_t wsb = mi_lightning_indexer_workspace(lqc, (int)B, (int)S1, rows, cap);
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(query.device()));
    const int rc = mi_lightning_indexer(
        query.data_ptr(), key.data_ptr(), w.data_ptr(), out.data_ptr<int>(), aq.has_value() ? aq->data_ptr<int>() : nullptr,
        ak.has_value() ? ak->data_ptr<int>() : nullptr, bt.has_value() ? bt->data_ptr<int>() : nullptr, lqc, lkc, (int)B, (int)S1, rows, (int)n1,
        (int)n2, (int)D, cap, (int)block_size, bt.has_value() ? bt->stride(0) : 0, query.stride(0), q_tnd ? 0 : query.stride(1),
        query.stride(qd - 2), w.stride(0), q_tnd ? 0 : w.stride(1), k_tnd ? 0 : key.stride(0), key.stride(k_tnd ? 0 : 1), (int)count, (int)mode,
        dtype_code(query), ws.data_ptr(), wsb, cur_stream());
    TORCH_CHECK(rc == 0, "mi_lightning_indexer failed with code ", rc, " (strides of query / key multiples of 8 elements, of weights of 4)");
    return out;
}

// csrc/sparse_attn_sharedkv/op_host/sparse_attn_sharedkv.cpp:49-200 (checks: the same file :60-114 and op_host/sparse_attn_sharedkv_tiling.cpp
// :1096-1257, :1406-1410, whose wording the messages keep where they have one): window + token-sparse attention over a shared 512-wide
// latent, the consumer of lightning_indexer's indices (csrc/kernels/sparse_sharedkv.hip; semantics in include/mi_sgl_kernels.h).  Returns
// (attention_out = empty_like(q) with every row written, an empty fp32 softmax_lse).  metadata (the reference's per-core schedule) is checked
// when given and never read; cu_seqlens_ori_kv / cu_seqlens_cmp_kv belong to the non-paged layouts and are ignored under PA_ND.
std::tuple<at::Tensor, at::Tensor> sparse_attn_sharedkv(
    const at::Tensor &q, const std::optional<at::Tensor> &ori_kv, const std::optional<at::Tensor> &cmp_kv,
    const std::optional<at::Tensor> &ori_sparse_indices, const std::optional<at::Tensor> &cmp_sparse_indices,
    const std::optional<at::Tensor> &ori_block_table, const std::optional<at::Tensor> &cmp_block_table,
    const std::optional<at::Tensor> &cu_seqlens_q, const std::optional<at::Tensor> &cu_seqlens_ori_kv,
    const std::optional<at::Tensor> &cu_seqlens_cmp_kv, const std::optional<at::Tensor> &seqused_q, const std::optional<at::Tensor> &seqused_kv,
    const std::optional<at::Tensor> &sinks, const std::optional<at::Tensor> &metadata, double softmax_scale, int64_t cmp_ratio,
    int64_t ori_mask_mode, int64_t cmp_mask_mode, int64_t ori_win_left, int64_t ori_win_right, c10::string_view layout_q,
    c10::string_view layout_kv, bool return_softmax_lse)
{
    const c10::DeviceGuard device_guard(q.device());   // launches and the current stream follow the tensor's GPU
    const bool tnd = layout_q == "TND";
    TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "sparse_attn_sharedkv: q must be float16 or bfloat16");
    TORCH_CHECK(layout_q == "BSND" || tnd, "sparse_attn_sharedkv: layout_q must be 'BSND' or 'TND'");
    TORCH_CHECK((!tnd && q.dim() == 4) || (tnd && q.dim() == 3), "sparse_attn_sharedkv: q rank does not match layout_q");
    TORCH_CHECK(ori_kv.has_value(), "sparse_attn_sharedkv: ori_kv is required");
    TORCH_CHECK(sinks.has_value(), "sparse_attn_sharedkv: sinks is required");
    TORCH_CHECK(layout_kv == "PA_ND", "sparse_attn_sharedkv: this port currently supports layout_kv='PA_ND' only");
    TORCH_CHECK(!return_softmax_lse, "sparse_attn_sharedkv: return_softmax_lse=true is not supported");
    TORCH_CHECK(!ori_sparse_indices.has_value(),
                "sparse_attn_sharedkv: ori_sparse_indices (a second gather over the original cache) is not supported here");
    TORCH_CHECK(ori_block_table.has_value(), "sparse_attn_sharedkv: ori_block_table is required for PA_ND");
    TORCH_CHECK(seqused_kv.has_value(), "sparse_attn_sharedkv: seqused_kv is required for PA_ND");
    TORCH_CHECK(!cmp_kv.has_value() || cmp_block_table.has_value(), "sparse_attn_sharedkv: cmp_block_table is required when cmp_kv is present");
    TORCH_CHECK(!cmp_sparse_indices.has_value() || cmp_kv.has_value(),
                "sparse_attn_sharedkv: cmp_kv is required when cmp_sparse_indices is present");
    TORCH_CHECK(!tnd || cu_seqlens_q.has_value(), "sparse_attn_sharedkv: cu_seqlens_q is required for TND query layout");
    TORCH_CHECK(tnd || !cu_seqlens_q.has_value(), "sparse_attn_sharedkv: cu_seqlens_q must be None for BSND query layout");
    TORCH_CHECK(ori_win_left >= 0 && ori_win_right >= 0, "sparse_attn_sharedkv: window sizes must be non-negative");
    TORCH_CHECK(ori_win_left <= INT32_MAX && ori_win_right <= INT32_MAX, "sparse_attn_sharedkv: integer attributes exceed the supported range");
    TORCH_CHECK(softmax_scale >= 0.0 && softmax_scale < HUGE_VAL, "sparse_attn_sharedkv: softmax_scale must be non-negative");
    TORCH_CHECK(ori_kv->scalar_type() == q.scalar_type(), "sparse_attn_sharedkv: ori_kv dtype must match q dtype");
    TORCH_CHECK(!cmp_kv.has_value() || cmp_kv->scalar_type() == q.scalar_type(), "sparse_attn_sharedkv: cmp_kv dtype must match q dtype");
    TORCH_CHECK(sinks->scalar_type() == at::kFloat, "sparse_attn_sharedkv: sinks must be float32");
    TORCH_CHECK(!metadata.has_value() || (metadata->scalar_type() == at::kInt && metadata->numel() == 1024),
                "sparse_attn_sharedkv: metadata must be int32 with 1024 elements");
    TORCH_CHECK(ori_mask_mode == 4, "sparse_attn_sharedkv: ori_mask_mode only supports 4");
    TORCH_CHECK(cmp_mask_mode == 3, "sparse_attn_sharedkv: cmp_mask_mode only supports 3");
    const int64_t heads = q.size(tnd ? 1 : 2), D = q.size(tnd ? 2 : 3);
    TORCH_CHECK(heads == 64, "sparse_attn_sharedkv: the initial port supports exactly 64 query heads");
    TORCH_CHECK(D == 512, "sparse_attn_sharedkv: head dim of q only supports 512");
    auto int32 = [](const std::optional<at::Tensor> &t, const char *name) {
        TORCH_CHECK(!t.has_value() || t->scalar_type() == at::kInt, name, " must be int32");
    };
    int32(cmp_sparse_indices, "cmp_sparse_indices"), int32(ori_block_table, "ori_block_table"), int32(cmp_block_table, "cmp_block_table");
    int32(cu_seqlens_q, "cu_seqlens_q"), int32(cu_seqlens_ori_kv, "cu_seqlens_ori_kv"), int32(cu_seqlens_cmp_kv, "cu_seqlens_cmp_kv");
    int32(seqused_q, "seqused_q"), int32(seqused_kv, "seqused_kv");
    auto same_device = [&](const std::optional<at::Tensor> &t, const char *name) {
        TORCH_CHECK(!t.has_value() || t->device() == q.device(), name, " must be on the same device as q");
    };
    same_device(ori_kv, "ori_kv"), same_device(cmp_kv, "cmp_kv"), same_device(cmp_sparse_indices, "cmp_sparse_indices");
    same_device(ori_block_table, "ori_block_table"), same_device(cmp_block_table, "cmp_block_table"), same_device(cu_seqlens_q, "cu_seqlens_q");
    same_device(seqused_q, "seqused_q"), same_device(seqused_kv, "seqused_kv"), same_device(sinks, "sinks");
    auto paged = [&](const at::Tensor &kv, const at::Tensor &table, const char *name) {
        TORCH_CHECK(kv.dim() == 4 && kv.size(2) == 1 && kv.size(3) == D, "sparse_attn_sharedkv: ", name, " must be [pages, block, 1, 512]");
        TORCH_CHECK(kv.size(1) > 0 && kv.size(1) <= 1024 && kv.size(1) % 16 == 0, "sparse_attn_sharedkv: block size of ", name,
                    " must be a multiple of 16 and belong to (0, 1024]");
        TORCH_CHECK(kv.stride(3) == 1 && kv.stride(1) == D && kv.stride(0) % 8 == 0, "sparse_attn_sharedkv: rows of ", name,
                    " must be contiguous and its page stride a multiple of 8 elements");
        TORCH_CHECK(table.dim() == 2 && table.size(1) > 0, "sparse_attn_sharedkv: the block table of ", name, " must be [batch, columns]");
    };
    paged(*ori_kv, *ori_block_table, "ori_kv");
    if (cmp_kv.has_value()) {
        paged(*cmp_kv, *cmp_block_table, "cmp_kv");
        TORCH_CHECK(cmp_ratio == 4 || cmp_ratio == 128, "sparse_attn_sharedkv: cmp_ratio only supports 4 or 128 when cmp_kv is present");
    }
    TORCH_CHECK(sinks->numel() == heads, "sparse_attn_sharedkv: sinks must hold one value per query head");
    const int64_t B = tnd ? cu_seqlens_q->numel() - 1 : q.size(0), S1 = tnd ? 1 : q.size(1), tokens = tnd ? q.size(0) : B * S1;
    TORCH_CHECK(B >= 0 && B <= INT32_MAX && S1 <= INT32_MAX, "sparse_attn_sharedkv: batch size");
    TORCH_CHECK(seqused_kv->numel() == B, "sparse_attn_sharedkv: seqused_kv's dimension should be equal to ", B);
    TORCH_CHECK(!seqused_q.has_value() || seqused_q->numel() == B, "sparse_attn_sharedkv: seqused_q's dimension should be equal to ", B);
    TORCH_CHECK(ori_block_table->size(0) == B && (!cmp_block_table.has_value() || cmp_block_table->size(0) == B),
                "sparse_attn_sharedkv: dim 0 of the block tables must be the batch size");
    int64_t K = 0;
    if (cmp_sparse_indices.has_value()) {
        const at::Tensor &ix = *cmp_sparse_indices;
        TORCH_CHECK(ix.dim() == q.dim() && ix.size(q.dim() - 2) == 1 && ix.size(0) == q.size(0) && (tnd || ix.size(1) == S1),
                    "sparse_attn_sharedkv: cmp_sparse_indices must be [B, S1, 1, K] (BSND) or [T, 1, K] (TND)");
        K = ix.size(q.dim() - 1);
        TORCH_CHECK(K >= 1 && K <= 2048, "sparse_attn_sharedkv: the sparse count K of cmp_sparse_indices must belong to [1, 2048], but now is ", K);
    }
    TORCH_CHECK(q.stride(q.dim() - 1) == 1 && q.stride(q.dim() - 2) % 8 == 0, "sparse_attn_sharedkv: q's innermost dimension must be contiguous");

    at::Tensor attention_out = at::empty_like(q);
    at::Tensor softmax_lse = at::empty({0}, q.options().dtype(at::kFloat));
    if (B == 0 || tokens == 0) return {attention_out, softmax_lse};
    auto contig = [](const std::optional<at::Tensor> &t) { return t.has_value() ? std::optional<at::Tensor>(t->contiguous()) : std::nullopt; };
    auto rows_contig = [&](const std::optional<at::Tensor> &t) { return t.has_value() && t->stride(t->dim() - 1) != 1 ? contig(t) : t; };
    const std::optional<at::Tensor> cu = contig(cu_seqlens_q), sq = contig(seqused_q), skv = contig(seqused_kv);
    const std::optional<at::Tensor> obt = rows_contig(ori_block_table), cbt = rows_contig(cmp_block_table), ix = rows_contig(cmp_sparse_indices);
    const at::Tensor sk = sinks->contiguous();
    auto i32 = [](const std::optional<at::Tensor> &t) { return t.has_value() ? t->data_ptr<int>() : nullptr; };
    const int64_t win = ori_win_left + ori_win_right + 1, ori_cap = obt->size(1) * ori_kv->size(1);
    const int64_t list_bound = std::min(win, ori_cap) + (ix.has_value() ? K : cmp_kv.has_value() ? cbt->size(1) * cmp_kv->size(1) : 0);
    const size_t wsb = mi_sparse_attn_sharedkv_workspace(tokens, list_bound, 0);
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(q.device()));
    const at::Tensor &o = attention_out;
    const int rc = mi_sparse_attn_sharedkv(
        q.data_ptr(), ori_kv->data_ptr(), cmp_kv.has_value() ? cmp_kv->data_ptr() : nullptr, o.data_ptr(), sk.data_ptr<float>(), i32(ix),
        i32(obt), i32(cbt), i32(cu), i32(sq), i32(skv), tnd ? MI_SSK_Q_TND : MI_SSK_Q_BSND, (int)B, (int)S1, tokens, (int)heads, (int)D,
        (int)ori_kv->size(1), (int)obt->size(1), cmp_kv.has_value() ? (int)cmp_kv->size(1) : 0, cbt.has_value() ? (int)cbt->size(1) : 0, (int)K,
        tnd ? 0 : q.stride(0), tnd ? q.stride(0) : q.stride(1), q.stride(q.dim() - 2), tnd ? 0 : o.stride(0), tnd ? o.stride(0) : o.stride(1),
        o.stride(o.dim() - 2), ix.has_value() && !tnd ? ix->stride(0) : 0, ix.has_value() ? ix->stride(tnd ? 0 : 1) : 0, ori_kv->stride(0),
        cmp_kv.has_value() ? cmp_kv->stride(0) : 0, obt->stride(0), cbt.has_value() ? cbt->stride(0) : 0, (float)softmax_scale, (int)cmp_ratio,
        (int)ori_win_left, (int)ori_win_right, dtype_code(q), 0, ws.data_ptr(), wsb, cur_stream());
    TORCH_CHECK(rc == 0, "mi_sparse_attn_sharedkv failed with code ", rc, " (strides of q / out multiples of 8 elements)");
    return {attention_out, softmax_lse};
}

// csrc/compressor/op_host/compressor.cpp:157-305 (checks: op_host/compressor_tiling.h:111-139, :215-225 and compressor_tiling.cpp:808-997):
// the KV compressor that produces the cache lightning_indexer and sparse_attn_sharedkv read (csrc/kernels/compressor.hip; semantics in
// include/mi_sgl_kernels.h).  Returns cmp_kv with every row written (rows no group fills are zeros); state_cache is updated in place.
// seqused = None: every token of a sequence exists; start_pos = None: zeros (GetSeqUsed / GetStartPos of the reference kernel).
at::Tensor compressor(const at::Tensor &x, const at::Tensor &wkv, const at::Tensor &wgate, at::Tensor &state_cache, const at::Tensor &ape,
                      const at::Tensor &norm_weight, const at::Tensor &rope_sin, const at::Tensor &rope_cos,
                      const std::optional<at::Tensor> &state_block_table, const std::optional<at::Tensor> &cu_seqlens,
                      const std::optional<at::Tensor> &seqused, const std::optional<at::Tensor> &start_pos, int64_t rope_head_dim,
                      int64_t cmp_ratio, int64_t coff, double norm_eps, int64_t rotary_mode, int64_t cache_mode,
                      int64_t state_cache_stride_dim0)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(x.scalar_type() == at::kHalf || x.scalar_type() == at::kBFloat16, "compressor: Tensor x only supports dtype float16 or bfloat16");
    TORCH_CHECK(wkv.scalar_type() == x.scalar_type() && wgate.scalar_type() == x.scalar_type(),
                "compressor: wkv and wgate datatype should be same with x");
    auto f32 = [](const at::Tensor &t, const char *name) { TORCH_CHECK(t.scalar_type() == at::kFloat, "compressor: Tensor ", name, " only supports dtype float32"); };
    f32(state_cache, "state_cache"), f32(ape, "ape"), f32(norm_weight, "norm_weight"), f32(rope_sin, "rope_sin"), f32(rope_cos, "rope_cos");
    auto i32 = [](const std::optional<at::Tensor> &t, const char *name) {
        TORCH_CHECK(!t.has_value() || t->scalar_type() == at::kInt, "compressor: Tensor ", name, " only supports dtype int32");
    };
    i32(state_block_table, "state_block_table"), i32(cu_seqlens, "cu_seqlens"), i32(seqused, "seqused"), i32(start_pos, "start_pos");
    auto same_device = [&](const at::Tensor &t, const char *name) { TORCH_CHECK(t.device() == x.device(), "compressor: ", name, " must be on the same device as x"); };
    same_device(wkv, "wkv"), same_device(wgate, "wgate"), same_device(state_cache, "state_cache"), same_device(ape, "ape");
    same_device(norm_weight, "norm_weight"), same_device(rope_sin, "rope_sin"), same_device(rope_cos, "rope_cos");
    for (const auto *t : {&state_block_table, &cu_seqlens, &seqused, &start_pos})
        if (t->has_value()) same_device(**t, "an int32 input");
    TORCH_CHECK(x.dim() == 2 || x.dim() == 3, "compressor: x dim number only supports 2 (TH) or 3 (BSH)");
    const bool th = x.dim() == 2;
    TORCH_CHECK(wkv.dim() == 2 && wgate.dim() == 2 && state_cache.dim() == 3 && ape.dim() == 2 && norm_weight.dim() == 1,
                "compressor: wkv, wgate and ape must be 2-dimensional, state_cache 3-dimensional, norm_weight 1-dimensional");
    TORCH_CHECK(rope_sin.dim() == x.dim() && rope_cos.dim() == x.dim(), "compressor: rope_sin / rope_cos dim num should be equal to x");
    TORCH_CHECK(state_block_table.has_value(), "compressor: tensor state_block_table is required");
    TORCH_CHECK(state_block_table->dim() == 1 || state_block_table->dim() == 2, "compressor: state_block_table must be 1- or 2-dimensional");
    TORCH_CHECK(!th || cu_seqlens.has_value(), "compressor: In TH layout, tensor cu_seqlens should not be None");
    TORCH_CHECK(th || !cu_seqlens.has_value(), "compressor: In BSH layout, tensor cu_seqlens must be None");
    TORCH_CHECK(!cu_seqlens.has_value() || (cu_seqlens->dim() == 1 && cu_seqlens->numel() >= 1), "compressor: cu_seqlens must be [batch + 1]");
    TORCH_CHECK(!seqused.has_value() || seqused->dim() == 1, "compressor: seqused must be 1-dimensional");
    TORCH_CHECK(!start_pos.has_value() || start_pos->dim() == 1, "compressor: start_pos must be 1-dimensional");
    TORCH_CHECK(coff == 1 || coff == 2, "compressor: coff only supports 1 or 2");
    TORCH_CHECK(cmp_ratio >= 1 && cmp_ratio <= 128, "compressor: cmp_ratio out of range");
    const int64_t D = norm_weight.size(0), H = x.size(x.dim() - 1), ww = coff * D;
    const int64_t B = th ? cu_seqlens->numel() - 1 : x.size(0), S = th ? 0 : x.size(1), T = th ? x.size(0) : B * S;
    TORCH_CHECK(B <= INT32_MAX && S <= INT32_MAX, "compressor: batch size");
    const int64_t cg = th ? 0 : (S + cmp_ratio - 1) / cmp_ratio, out_rows = th ? std::min(T, T / cmp_ratio + B) : B * cg;
    auto dim_is = [](const at::Tensor &t, int64_t dim, int64_t want, const char *name, const char *what) {
        TORCH_CHECK(t.size(dim) == want, "compressor: ", name, " shape dim ", dim, " should be equal to ", what, ": ", want, ", but got ", t.size(dim));
    };
    dim_is(wkv, 1, H, "wkv", "hiddenSize"), dim_is(wgate, 1, H, "wgate", "hiddenSize");
    dim_is(wkv, 0, ww, "wkv", "coff*headDim"), dim_is(wgate, 0, ww, "wgate", "coff*headDim");
    dim_is(state_cache, 2, 2 * ww, "state_cache", "2*coff*headDim");
    dim_is(ape, 1, ww, "ape", "coff*headDim"), dim_is(ape, 0, cmp_ratio, "ape", "cmpRatio");
    dim_is(*state_block_table, 0, B, "state_block_table", "batchSize");
    if (seqused.has_value()) dim_is(*seqused, 0, B, "seqused", "batchSize");
    if (start_pos.has_value()) dim_is(*start_pos, 0, B, "start_pos", "batchSize");
    if (th) {
        dim_is(rope_sin, 0, out_rows, "rope_sin", "min(tokenSize, tokenSize/cmpRatio+batchSize)");
        dim_is(rope_cos, 0, out_rows, "rope_cos", "min(tokenSize, tokenSize/cmpRatio+batchSize)");
        dim_is(rope_sin, 1, rope_head_dim, "rope_sin", "ropeHeadDim"), dim_is(rope_cos, 1, rope_head_dim, "rope_cos", "ropeHeadDim");
    } else {
        dim_is(rope_sin, 0, B, "rope_sin", "batchSize"), dim_is(rope_cos, 0, B, "rope_cos", "batchSize");
        dim_is(rope_sin, 1, cg, "rope_sin", "ceil(seqSize/cmpRatio)"), dim_is(rope_cos, 1, cg, "rope_cos", "ceil(seqSize/cmpRatio)");
        dim_is(rope_sin, 2, rope_head_dim, "rope_sin", "ropeHeadDim"), dim_is(rope_cos, 2, rope_head_dim, "rope_cos", "ropeHeadDim");
    }
    TORCH_CHECK(state_cache.is_contiguous(), "compressor: state_cache must be contiguous");

    at::Tensor cmp_kv = th ? at::empty({out_rows, D}, x.options()) : at::empty({B, cg, D}, x.options());
    const bool launch = T > 0 && B > 0;
    const at::Tensor xc = x.contiguous(), wk = wkv.contiguous(), wg = wgate.contiguous(), ap = ape.contiguous(), nw = norm_weight.contiguous();
    const at::Tensor rs = rope_sin.contiguous(), rc = rope_cos.contiguous();
    auto contig = [](const std::optional<at::Tensor> &t) { return t.has_value() ? std::optional<at::Tensor>(t->contiguous()) : std::nullopt; };
    const std::optional<at::Tensor> tb = contig(state_block_table), cu = contig(cu_seqlens), su = contig(seqused), sp = contig(start_pos);
    auto iptr = [](const std::optional<at::Tensor> &t) { return t.has_value() ? t->data_ptr<int>() : nullptr; };
    const size_t wsb = launch ? mi_compressor_workspace(T, (int)B, (int)H, (int)D, (int)coff) : 0;
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(x.device()));
    mi_compressor_params p{};
    p.x = xc.data_ptr(), p.wkv = wk.data_ptr(), p.wgate = wg.data_ptr(), p.state_cache = state_cache.data_ptr<float>();
    p.ape = ap.data_ptr<float>(), p.norm_weight = nw.data_ptr<float>(), p.rope_sin = rs.data_ptr<float>(), p.rope_cos = rc.data_ptr<float>();
    p.state_block_table = iptr(tb), p.cu_seqlens = iptr(cu), p.seqused = iptr(su), p.start_pos = iptr(sp);
    p.cmp_kv = cmp_kv.data_ptr(), p.workspace = ws.data_ptr(), p.workspace_bytes = wsb;
    p.tokens = T, p.out_rows = out_rows, p.state_blocks = state_cache.size(0), p.table_stride = tb->dim() == 2 ? tb->stride(0) : 1;
    p.state_cache_stride_dim0 = state_cache_stride_dim0;
    p.layout = th ? MI_COMPRESSOR_TH : MI_COMPRESSOR_BSH, p.batch = (int)B, p.seq = (int)S, p.hidden = (int)std::min<int64_t>(H, INT32_MAX);
    p.head_dim = (int)std::min<int64_t>(D, INT32_MAX), p.cmp_ratio = (int)cmp_ratio, p.coff = (int)coff;
    p.rope_head_dim = (int)std::min<int64_t>(std::max<int64_t>(rope_head_dim, 0), INT32_MAX);
    p.rotary_mode = (int)std::min<int64_t>(std::max<int64_t>(rotary_mode, -1), 64), p.cache_mode = (int)std::min<int64_t>(std::max<int64_t>(cache_mode, -1), 64);
    p.block_size = (int)std::min<int64_t>(state_cache.size(1), INT32_MAX), p.table_dims = (int)tb->dim();
    p.table_cols = tb->dim() == 2 ? (int)std::min<int64_t>(tb->size(1), INT32_MAX) : 1, p.dtype = dtype_code(x), p.norm_eps = (float)norm_eps;
    const int rc_ = mi_compressor(&p, cur_stream());
    TORCH_CHECK(rc_ == 0, "mi_compressor failed with code ", rc_,
                " ((cmp_ratio, coff, head_dim) must be (4, 2, 512), (4, 2, 128) or (128, 1, 512); 1024 <= hidden <= 10240 and a multiple of 512; "
                "rope_head_dim 64; rotary_mode 1 or 2; cache_mode 1 or 2, in mode 2 a 2-D table of at least coff*cmp_ratio+1 columns; "
                "state_cache_stride_dim0 0 or size(1)*size(2))");
    return cmp_kv;
}

// csrc/sparse_attention_score/ (op_host/sparse_attention_score.cpp): block-sparse GQA attention over per-token block lists, the reference's
// native main-attention op (csrc/kernels/sparse_attention_score.hip; semantics in include/mi_sgl_kernels.h).  Shapes override the
// attributes: Hkv, Q and topK come from select_idx, batch and columns from block_table; scale_value within 1e-9 of zero means 1 / sqrt(D).
// inner_precise is accepted and every value runs the high-precision path (fp32 scores, softmax and accumulation).  Nothing is copied to or
// read back from the device: only the output and the workspace are allocated, from shapes.
at::Tensor npu_sparse_attention_score(const at::Tensor &query, const at::Tensor &key, const at::Tensor &value, const at::Tensor &select_idx,
                                      const at::Tensor &block_table, const std::optional<at::Tensor> &select_num_idx,
                                      const std::optional<at::Tensor> &q_dequant_scale, const std::optional<at::Tensor> &k_dequant_scale,
                                      const std::optional<at::Tensor> &v_dequant_scale, const std::optional<at::Tensor> &actual_seq_lengths,
                                      const std::optional<at::Tensor> &actual_seq_lengths_kv, int64_t num_key_value_heads, double scale_value,
                                      int64_t block_size, int64_t top_k, int64_t inner_precise)
{
    (void)num_key_value_heads, (void)top_k, (void)inner_precise;
    const c10::DeviceGuard device_guard(query.device());
    const auto qt = query.scalar_type();
    const bool fp8 = qt == at::kFloat8_e4m3fn;
    TORCH_CHECK(qt == at::kHalf || qt == at::kBFloat16 || fp8, "npu_sparse_attention_score: query must be bf16, fp16 or float8_e4m3fn");
    TORCH_CHECK(key.scalar_type() == qt, "npu_sparse_attention_score: key must have the query's dtype");
    TORCH_CHECK(value.scalar_type() == qt, "npu_sparse_attention_score: value must have the query's dtype");
    TORCH_CHECK(select_idx.scalar_type() == at::kInt, "npu_sparse_attention_score: select_idx must be int32");
    TORCH_CHECK(block_table.scalar_type() == at::kInt, "npu_sparse_attention_score: block_table must be int32");
    TORCH_CHECK(actual_seq_lengths_kv.has_value(), "npu_sparse_attention_score: actual_seq_lengths_kv is required");
    auto same_device = [&](const at::Tensor &t, const char *name) {
        TORCH_CHECK(t.device() == query.device(), "npu_sparse_attention_score: ", name, " must be on the query's device");
    };
    auto optional_i32 = [&](const std::optional<at::Tensor> &t, const char *name) {
        if (!t.has_value()) return;
        TORCH_CHECK(t->scalar_type() == at::kInt, "npu_sparse_attention_score: ", name, " must be int32");
        same_device(*t, name);
    };
    same_device(key, "key"), same_device(value, "value"), same_device(select_idx, "select_idx"), same_device(block_table, "block_table");
    optional_i32(select_num_idx, "select_num_idx"), optional_i32(actual_seq_lengths, "actual_seq_lengths");
    optional_i32(actual_seq_lengths_kv, "actual_seq_lengths_kv");
    TORCH_CHECK(query.dim() == 3, "npu_sparse_attention_score: query must be [T, Hq, D]");
    TORCH_CHECK(key.dim() == 4, "npu_sparse_attention_score: key must be [pages, block_size, Hkv, D]");
    TORCH_CHECK(value.dim() == 4, "npu_sparse_attention_score: value must be [pages, block_size, Hkv, D]");
    TORCH_CHECK(select_idx.dim() == 3, "npu_sparse_attention_score: select_idx must be [Hkv, Q, topK]");
    TORCH_CHECK(block_table.dim() == 2, "npu_sparse_attention_score: block_table must be [batch, columns]");
    const int64_t T = query.size(0), Hq = query.size(1), D = query.size(2);
    const int64_t Hkv = select_idx.size(0), Q = select_idx.size(1), topk = select_idx.size(2);
    const int64_t batch = block_table.size(0), columns = block_table.size(1);
    TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "npu_sparse_attention_score: query heads (", Hq, ") must be a multiple of select_idx.size(0) (", Hkv, ")");
    TORCH_CHECK(key.sizes() == value.sizes(), "npu_sparse_attention_score: key and value shapes differ");
    TORCH_CHECK(key.size(2) == Hkv, "npu_sparse_attention_score: key.size(2) must equal select_idx.size(0)");
    TORCH_CHECK(key.size(3) == D, "npu_sparse_attention_score: key.size(3) must equal the query's head dim");
    TORCH_CHECK(block_size == key.size(1) && (block_size == 16 || block_size == 32 || block_size == 64 || block_size == 128),
                "npu_sparse_attention_score: block_size must equal key.size(1) and be 16, 32, 64 or 128");
    TORCH_CHECK(D > 0 && D % 8 == 0 && D <= 256, "npu_sparse_attention_score: query head dim must be a multiple of 8 up to 256");
    TORCH_CHECK(!fp8 || (D == 128 && block_size == 128), "npu_sparse_attention_score: a float8_e4m3fn query needs head dim 128 and block_size 128");
    TORCH_CHECK(Q >= T, "npu_sparse_attention_score: select_idx.size(1) (", Q, ") must cover the query's tokens (", T, ")");
    TORCH_CHECK(topk >= 1 && topk <= 1024, "npu_sparse_attention_score: select_idx.size(2) (topK) must be in [1, 1024]");
    TORCH_CHECK(!select_num_idx.has_value() || (select_num_idx->dim() == 2 && select_num_idx->size(0) == Hkv && select_num_idx->size(1) == Q),
                "npu_sparse_attention_score: select_num_idx must be [Hkv, Q]");
    TORCH_CHECK(!actual_seq_lengths.has_value() || actual_seq_lengths->numel() == batch,
                "npu_sparse_attention_score: actual_seq_lengths must have block_table.size(0) elements");
    TORCH_CHECK(actual_seq_lengths.has_value() || T == batch || T == 0,
                "npu_sparse_attention_score: without actual_seq_lengths every request has one token: T must equal block_table.size(0)");
    TORCH_CHECK(actual_seq_lengths_kv->numel() == batch, "npu_sparse_attention_score: actual_seq_lengths_kv must have block_table.size(0) elements");
    auto scale_arg = [&](const std::optional<at::Tensor> &t, const char *name, int64_t heads, int64_t last) {
        TORCH_CHECK(t.has_value() == fp8, "npu_sparse_attention_score: ", name, fp8 ? " is required with a float8_e4m3fn query" : " is only taken with a float8_e4m3fn query");
        if (!fp8) return;
        same_device(*t, name);
        TORCH_CHECK(t->scalar_type() == at::kFloat && t->dim() == 3 && t->size(0) == batch && t->size(1) == heads && (last < 0 ? t->size(2) >= 1 : t->size(2) == last),
                    "npu_sparse_attention_score: ", name, " must be fp32 [batch, heads, blocks]");
    };
    scale_arg(q_dequant_scale, "q_dequant_scale", Hq, -1);
    scale_arg(k_dequant_scale, "k_dequant_scale", Hkv, columns);
    scale_arg(v_dequant_scale, "v_dequant_scale", Hkv, columns);
    TORCH_CHECK(query.stride(2) == 1 && key.stride(3) == 1 && value.stride(3) == 1, "npu_sparse_attention_score: the innermost dimension of query, key and value must be contiguous");
    const double scale = std::fabs(scale_value) <= 1e-9 ? 1.0 / std::sqrt((double)D) : scale_value;
    TORCH_CHECK(scale > 0, "npu_sparse_attention_score: scale_value must be positive (or 0 for 1 / sqrt(D))");

    at::Tensor out = at::empty({T, Hq, D}, query.options().dtype(fp8 ? at::kHalf : qt));
    if (T == 0 || batch == 0) return out.zero_();
    const int chunks = mi_sparse_attention_score_num_chunks(T, (int)Hkv, (int)topk);
    const size_t wsb = mi_sparse_attention_score_workspace(T, (int)Hq, (int)D, chunks);
    at::Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 16)}, at::dtype(at::kByte).device(query.device()));
    // contiguous() copies on the device, in stream order, only where a view is passed
    const at::Tensor qlen = actual_seq_lengths.has_value() ? actual_seq_lengths->contiguous() : at::Tensor();
    const at::Tensor kvlen = actual_seq_lengths_kv->contiguous();
    at::Tensor sq, sk, sv;
    if (fp8) sq = q_dequant_scale->contiguous(), sk = k_dequant_scale->contiguous(), sv = v_dequant_scale->contiguous();
    mi_sparse_attention_score_params p{};
    p.q = query.data_ptr(), p.k = key.data_ptr(), p.v = value.data_ptr(), p.out = out.data_ptr();
    p.select_idx = select_idx.data_ptr<int>(), p.select_num_idx = select_num_idx.has_value() ? select_num_idx->data_ptr<int>() : nullptr;
    p.block_table = block_table.data_ptr<int>(), p.actual_seq_lengths = qlen.defined() ? qlen.data_ptr<int>() : nullptr;
    p.actual_seq_lengths_kv = kvlen.data_ptr<int>();
    if (fp8) p.q_dequant_scale = sq.data_ptr<float>(), p.k_dequant_scale = sk.data_ptr<float>(), p.v_dequant_scale = sv.data_ptr<float>();
    p.workspace = ws.data_ptr(), p.workspace_bytes = wsb, p.tokens = T;
    p.q_stride_t = query.stride(0), p.q_stride_h = query.stride(1), p.k_stride_blk = key.stride(0), p.k_stride_row = key.stride(1), p.k_stride_h = key.stride(2);
    p.v_stride_blk = value.stride(0), p.v_stride_row = value.stride(1), p.v_stride_h = value.stride(2), p.o_stride_t = out.stride(0), p.o_stride_h = out.stride(1);
    p.idx_stride_h = select_idx.stride(0), p.idx_stride_q = select_idx.stride(1), p.idx_stride_k = select_idx.stride(2);
    if (select_num_idx.has_value()) p.num_stride_h = select_num_idx->stride(0), p.num_stride_q = select_num_idx->stride(1);
    p.bt_stride_b = block_table.stride(0), p.bt_stride_n = block_table.stride(1);
    p.batch = (int)batch, p.q_heads = (int)Hq, p.kv_heads = (int)Hkv, p.head_dim = (int)D, p.block_size = (int)block_size, p.topk = (int)topk;
    p.columns = (int)std::min<int64_t>(columns, INT32_MAX), p.num_pages = (int)std::min<int64_t>(key.size(0), INT32_MAX);
    p.q_scale_blocks = fp8 ? (int)std::min<int64_t>(sq.size(2), INT32_MAX) : 0;
    p.dtype = fp8 ? MI_DTYPE_FP8_E4M3 : dtype_code(query), p.num_chunks = chunks, p.sm_scale = (float)scale;
    const int rc = mi_sparse_attention_score(&p, cur_stream());
    TORCH_CHECK(rc == 0, "mi_sparse_attention_score failed with code ", rc,
                " (strides of query multiples of 8 elements, of key / value multiples of 8 -- float8: 16 -- elements; 16-byte aligned tensors)");
    return out;
}

// SwiGLU + per-row INT8 quantisation; same arguments / returns as swiglu_quant (activation/swiglu_quant.py:87-127).
std::tuple<at::Tensor, at::Tensor> swiglu_quant(const at::Tensor &x, const at::Tensor &group_list, int64_t group_list_type,
                                                bool need_quant, bool do_limit, double limit)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(group_list_type == 0 || group_list_type == 1, "group_list_type must be 0 or 1, but got ", group_list_type);
    TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "swiglu_quant: x must be a contiguous [s, h] tensor");
    TORCH_CHECK(group_list.scalar_type() == at::kInt || group_list.scalar_type() == at::kLong,
                "group_list dtype must be torch.int32 or torch.int64, but got ", group_list.scalar_type());
    TORCH_CHECK(group_list.dim() == 1 && group_list.is_contiguous(), "swiglu_quant: group_list must be 1-D contiguous");
    const int64_t s = x.size(0), h = x.size(1);
    at::Tensor out = at::empty({s, h / 2}, x.options().dtype(need_quant ? at::kChar : x.scalar_type()));
    at::Tensor scale = at::empty({s}, x.options().dtype(at::kFloat));
    const int rc = mi_swiglu_quant(x.data_ptr(), group_list.data_ptr(), group_list.scalar_type() == at::kLong,
                                   (int)group_list.size(0), (int)group_list_type, (int)s, (int)h, need_quant, do_limit,
                                   (float)limit, dtype_code(x), out.data_ptr(), scale.data_ptr<float>(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_swiglu_quant failed with code ", rc, " (h must be a multiple of 16 and <= 8192)");
    return {out, scale};
}

// Fused Add + RMSNorm (+bias) (+static INT8 quant); returns (output, residual_sum) like add_rmsnorm_bias
// (norm/add_rmsnorm_bias.py:83-147).  gemma = true gives add_gemma_rms_norm (:194-232) which returns (norm, add_output).
std::tuple<at::Tensor, at::Tensor> add_rmsnorm_bias(const at::Tensor &input, const std::optional<at::Tensor> &residual,
                                                    const at::Tensor &norm_weight, const std::optional<at::Tensor> &norm_bias,
                                                    double eps, const std::optional<at::Tensor> &quant_scale,
                                                    const std::optional<at::Tensor> &quant_offset, bool gemma)
{
    const c10::DeviceGuard device_guard(input.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(input.dim() == 2 && input.stride(1) == 1, "add_rmsnorm_bias: input must be [batch, hidden] with contiguous rows");
    const int64_t B = input.size(0), H = input.size(1);
    TORCH_CHECK(norm_weight.numel() == H && norm_weight.is_contiguous() && norm_weight.scalar_type() == input.scalar_type(),
                "add_rmsnorm_bias: weight must be [hidden] in the input dtype");
    TORCH_CHECK(quant_scale.has_value() == quant_offset.has_value(), "quant_scale and quant_offset go together");
    at::Tensor res_c;
    if (residual.has_value()) {
        TORCH_CHECK(residual->sizes() == input.sizes() && residual->scalar_type() == input.scalar_type(), "residual shape/dtype");
        res_c = (residual->stride(0) == input.stride(0) && residual->stride(1) == 1) ? *residual : residual->contiguous();
    }
    at::Tensor in_c = input;
    if (residual.has_value() && res_c.stride(0) != input.stride(0)) in_c = input.contiguous(), res_c = res_c.contiguous();
    at::Tensor out = at::empty({B, H}, input.options().dtype(quant_scale.has_value() ? at::kChar : input.scalar_type()));
    at::Tensor out2 = residual.has_value() ? at::empty({B, H}, input.options()) : input;
    auto opt_ptr = [&](const std::optional<at::Tensor> &t) -> const void * {
        if (!t.has_value()) return nullptr;
        TORCH_CHECK(t->numel() == H && t->is_contiguous() && t->scalar_type() == input.scalar_type(),
                    "add_rmsnorm_bias: per-column vectors must be [hidden] in the input dtype");
        return t->data_ptr();
    };
    const int rc = mi_add_rmsnorm_bias(in_c.data_ptr(), residual.has_value() ? res_c.data_ptr() : nullptr, norm_weight.data_ptr(),
                                       opt_ptr(norm_bias), (float)eps, opt_ptr(quant_scale), opt_ptr(quant_offset), gemma, (int)B,
                                       (int)H, in_c.stride(0), dtype_code(input), out.data_ptr(),
                                       residual.has_value() ? out2.data_ptr() : nullptr, cur_stream());
    TORCH_CHECK(rc == 0, "mi_add_rmsnorm_bias failed with code ", rc, " (hidden must be a multiple of 8 and <= 8192)");
    return {out, out2};
}

// RoPE on q and the shared key heads; arguments / returns of fused_rope_qk_mqa (norm/fused_rope_qk_mqa.py:113-160).
std::tuple<at::Tensor, at::Tensor> fused_rope_qk_mqa(const at::Tensor &query, const at::Tensor &key, const at::Tensor &cos_sin,
                                                     int64_t rotary_dim, bool is_neox_style)
{
    const c10::DeviceGuard device_guard(query.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(query.dim() == 3 && key.dim() == 3 && cos_sin.dim() == 2, "fused_rope_qk_mqa: query [T,Hq,D], key [T,Hk,D], cos_sin [T,R]");
    TORCH_CHECK(query.size(0) == key.size(0) && query.size(2) == key.size(2) && cos_sin.size(0) >= query.size(0) &&
                    cos_sin.size(1) >= rotary_dim, "fused_rope_qk_mqa: shape mismatch");
    TORCH_CHECK(query.stride(2) == 1 && key.stride(2) == 1 && cos_sin.stride(1) == 1, "fused_rope_qk_mqa: innermost dims must be contiguous");
    TORCH_CHECK(query.scalar_type() == key.scalar_type() && query.scalar_type() == cos_sin.scalar_type(), "fused_rope_qk_mqa: dtype mismatch");
    at::Tensor out_q = at::empty(query.sizes(), query.options()), out_k = at::empty(key.sizes(), key.options());
    const int rc = mi_rope_qk_mqa(query.data_ptr(), key.data_ptr(), cos_sin.data_ptr(), (int)query.size(0), (int)query.size(1),
                                  (int)key.size(1), (int)query.size(2), (int)rotary_dim, is_neox_style, query.stride(0), query.stride(1),
                                  key.stride(0), key.stride(1), cos_sin.stride(0), dtype_code(query), out_q.data_ptr(), out_k.data_ptr(),
                                  cur_stream());
    TORCH_CHECK(rc == 0, "mi_rope_qk_mqa failed with code ", rc);
    return {out_q, out_k};
}

// split QKV + per-head RMSNorm + RoPE; arguments as split_qkv_rmsnorm_rope (norm/split_qkv_rmsnorm_rope.py:374-438).
std::tuple<at::Tensor, at::Tensor, at::Tensor> split_qkv_rmsnorm_rope(
    const at::Tensor &input, const at::Tensor &sin, const at::Tensor &cos, int64_t q_hidden_size, int64_t kv_hidden_size,
    int64_t head_dim, std::optional<double> eps, const std::optional<at::Tensor> &q_weight,
    const std::optional<at::Tensor> &k_weight, const std::optional<at::Tensor> &q_bias, const std::optional<at::Tensor> &k_bias,
    bool is_neox_style)
{
    const c10::DeviceGuard device_guard(input.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(input.dim() == 2 && input.is_contiguous(), "split_qkv_rmsnorm_rope: input must be contiguous [batch, q+2kv]");
    TORCH_CHECK((head_dim & (head_dim - 1)) == 0, "head_dim must be a power of two");        // reference :390-391
    TORCH_CHECK(q_hidden_size % kv_hidden_size == 0, "q_hidden_size % kv_hidden_size != 0");   // reference :392
    TORCH_CHECK(input.size(1) == q_hidden_size + 2 * kv_hidden_size, "split_qkv_rmsnorm_rope: input width");
    const int64_t B = input.size(0);
    const int64_t rope_dim = sin.size(-1);
    TORCH_CHECK(sin.numel() == B * rope_dim && cos.numel() == B * rope_dim && sin.is_contiguous() && cos.is_contiguous() &&
                    sin.scalar_type() == input.scalar_type() && cos.scalar_type() == input.scalar_type(),
                "split_qkv_rmsnorm_rope: sin/cos must be contiguous [batch, ..., rope_dim] in the input dtype");
    if (eps.has_value()) TORCH_CHECK(q_weight.has_value() && k_weight.has_value(), "norm weights are required when eps is given");
    TORCH_CHECK(q_bias.has_value() == k_bias.has_value(), "q_bias and k_bias go together");
    at::Tensor q = at::empty({B, q_hidden_size}, input.options()), k = at::empty({B, kv_hidden_size}, input.options()),
               v = at::empty({B, kv_hidden_size}, input.options());
    auto p = [](const std::optional<at::Tensor> &t) -> const void * { return t.has_value() ? t->data_ptr() : nullptr; };
    const int rc = mi_split_qkv_rmsnorm_rope(input.data_ptr(), sin.data_ptr(), cos.data_ptr(), (int)B, (int)q_hidden_size,
                                             (int)kv_hidden_size, (int)head_dim, (int)rope_dim, eps.has_value(),
                                             (float)eps.value_or(0.0), p(q_weight), p(k_weight), p(q_bias), p(k_bias),
                                             is_neox_style, dtype_code(input), q.data_ptr(), k.data_ptr(), v.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_split_qkv_rmsnorm_rope failed with code ", rc);
    return {q, k, v};
}

// norm/l1_norm.py:29-38: fp32 [batch, hidden] = input / sum(input, -1)
at::Tensor l1_norm(const at::Tensor &input)
{
    const c10::DeviceGuard device_guard(input.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(input.dim() == 2 && input.is_contiguous(), "l1_norm: input must be contiguous [batch, hidden]");
    at::Tensor out = at::empty(input.sizes(), input.options().dtype(at::kFloat));
    const int rc = mi_l1_norm(input.data_ptr(), input.size(0), (int)input.size(1), dtype_code3(input), out.data_ptr<float>(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_l1_norm failed with code ", rc);
    return out;
}

// norm/rmsnorm_without_weight.py:59-76: x [B, L, C] -> x * rsqrt(mean(x^2, -1) + eps), same dtype
at::Tensor rmsnorm_without_weight(const at::Tensor &x, double eps)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(x.dim() >= 1 && x.is_contiguous(), "fused_rmsnorm_without_weight: x must be contiguous");
    at::Tensor out = at::empty_like(x);
    const int64_t cols = x.size(-1);
    const int rc = mi_rmsnorm_without_weight(x.data_ptr(), cols ? x.numel() / cols : 0, (int)cols, (float)eps, dtype_code3(x), out.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_rmsnorm_without_weight failed with code ", rc);
    return out;
}

// norm/rmsnorm_split.py:150-161: x [B, L, C] -> mean(x^2, -1) as [B, L, 1] in x's dtype
at::Tensor fused_variance(const at::Tensor &x)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(x.dim() == 3 && x.is_contiguous(), "fused_variance: x must be contiguous [B, L, C]");
    at::Tensor out = at::empty({x.size(0), x.size(1), 1}, x.options());
    const int rc = mi_row_variance(x.data_ptr(), x.size(0) * x.size(1), (int)x.size(2), dtype_code3(x), out.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_row_variance failed with code ", rc);
    return out;
}

// norm/rmsnorm_split.py:76-97: x [B, L, C], variance [B * L], weight [C] -> x * rsqrt(variance + eps) * weight in x's dtype
at::Tensor fused_rsqrt_mul(const at::Tensor &x, const at::Tensor &variance, const at::Tensor &weight, double eps)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(x.dim() == 3 && x.is_contiguous(), "fused_rsqrt_mul: x must be contiguous [B, L, C]");
    const int64_t rows = x.size(0) * x.size(1), cols = x.size(2);
    TORCH_CHECK(variance.numel() == rows && variance.is_contiguous() && variance.scalar_type() == x.scalar_type(),
                "fused_rsqrt_mul: variance must hold B * L values in x's dtype");
    TORCH_CHECK(weight.numel() == cols && weight.is_contiguous() && weight.scalar_type() == x.scalar_type(),
                "fused_rsqrt_mul: weight must hold C values in x's dtype");
    at::Tensor out = at::empty_like(x);
    const int rc = mi_rsqrt_mul(x.data_ptr(), variance.data_ptr(), weight.data_ptr(), rows, (int)cols, (float)eps, dtype_code3(x), out.data_ptr(),
                                cur_stream());
    TORCH_CHECK(rc == 0, "mi_rsqrt_mul failed with code ", rc);
    return out;
}

// norm/scale_shift.py:122-183: x [B, L, C] * (c + scale) + shift
at::Tensor fused_scale_shift(const at::Tensor &x, const at::Tensor &scale, const at::Tensor &shift, double scale_constant)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(x.dim() == 3 && x.is_contiguous(), "fused_scale_shift: x must be contiguous [B, L, C]");
    TORCH_CHECK(scale.is_contiguous() && shift.is_contiguous() && scale.scalar_type() == shift.scalar_type() &&
                    (scale.scalar_type() == x.scalar_type() || scale.scalar_type() == at::kFloat),
                "fused_scale_shift: scale and shift must be contiguous, of one dtype: x's or float32");
    const int64_t rows = x.size(0) * x.size(1), cols = x.size(2);
    TORCH_CHECK(scale.numel() == 1 || scale.numel() == cols, "scale must be scalar or [hidden_size]");                               // reference :136-138
    TORCH_CHECK(shift.numel() == 1 || shift.numel() == cols || shift.numel() == x.numel(), "shift must be scalar, [hidden_size] or x's size");      // :139-141
    at::Tensor out = at::empty_like(x);
    const int rc = mi_scale_shift(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), rows, (int)cols, scale.numel(), shift.numel(), (float)scale_constant,
                                  dtype_code3(x), dtype_code3(scale), out.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_scale_shift failed with code ", rc);
    return out;
}

// norm/split_qkv_rmsnorm_mrope.py:335-420 (triton_split_qkv_rmsnorm_mrope)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> split_qkv_rmsnorm_mrope(
    const at::Tensor &qkv, const at::Tensor &q_weight, const at::Tensor &k_weight, const at::Tensor &cos_sin, int64_t num_q_heads,
    int64_t num_kv_heads, int64_t head_size, double eps, at::IntArrayRef mrope_section, bool is_interleaved, std::optional<int64_t> rope_dim_opt,
    const std::optional<at::Tensor> &q_bias, const std::optional<at::Tensor> &k_bias, bool has_gate)
{
    const c10::DeviceGuard device_guard(qkv.device());   // launches and the current stream follow the tensor's GPU
    const int64_t q_size = num_q_heads * head_size, kv_size = num_kv_heads * head_size, gate_size = has_gate ? q_size : 0;
    const int64_t rope_dim = rope_dim_opt.value_or(head_size);
    TORCH_CHECK(qkv.dim() == 2 && qkv.is_contiguous() && qkv.size(1) == q_size + gate_size + 2 * kv_size,
                "split_qkv_rmsnorm_mrope: qkv must be contiguous [tokens, q (+ gate) + 2 kv]");
    const int64_t T = qkv.size(0);
    TORCH_CHECK(mrope_section.size() == 3, "mrope_section must hold three section sizes");
    TORCH_CHECK(cos_sin.dim() == 3 && cos_sin.size(0) == 3 && cos_sin.size(1) == T && cos_sin.size(2) == rope_dim && cos_sin.is_contiguous() &&
                    cos_sin.scalar_type() == qkv.scalar_type(),
                "split_qkv_rmsnorm_mrope: cos_sin must be contiguous [3, tokens, rope_dim] in the input dtype");
    TORCH_CHECK(q_weight.numel() == head_size && k_weight.numel() == head_size && q_weight.scalar_type() == qkv.scalar_type() &&
                    k_weight.scalar_type() == qkv.scalar_type() && q_weight.is_contiguous() && k_weight.is_contiguous(),
                "split_qkv_rmsnorm_mrope: weights must be [head_size] in the input dtype");
    TORCH_CHECK(q_bias.has_value() == k_bias.has_value(), "q_bias and k_bias go together");
    TORCH_CHECK((head_size & (head_size - 1)) == 0 && head_size >= 64 && head_size <= 256 && rope_dim % 16 == 0 && rope_dim <= head_size,
                "split_qkv_rmsnorm_mrope: head_size must be 64, 128 or 256 and rope_dim a multiple of 16 (this build)");
    at::Tensor q = at::empty({T, q_size}, qkv.options()), k = at::empty({T, kv_size}, qkv.options()), v = at::empty({T, kv_size}, qkv.options()),
               gate = at::empty({T, gate_size}, qkv.options());
    auto p = [](const std::optional<at::Tensor> &t) -> const void * { return t.has_value() ? t->data_ptr() : nullptr; };
    const int rc = mi_split_qkv_rmsnorm_mrope(qkv.data_ptr(), cos_sin.data_ptr(), (int)T, (int)q_size, (int)kv_size, (int)head_size, (int)rope_dim,
                                              (float)eps, q_weight.data_ptr(), k_weight.data_ptr(), p(q_bias), p(k_bias), (int)mrope_section[0],
                                              (int)mrope_section[1], (int)mrope_section[2], is_interleaved, dtype_code(qkv), q.data_ptr(),
                                              k.data_ptr(), v.data_ptr(), has_gate ? gate.data_ptr() : nullptr, cur_stream());
    TORCH_CHECK(rc == 0, "mi_split_qkv_rmsnorm_mrope failed with code ", rc);
    return {q, k, v, gate};
}

// activation/swiglu_oai.py:53-83 (swiglu_oai_triton)
at::Tensor swiglu_oai(const at::Tensor &hidden_states, int64_t dim, double gemm1_alpha, double gemm1_clamp_limit)
{
    const c10::DeviceGuard device_guard(hidden_states.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(hidden_states.is_contiguous() && dim > 0 && dim % 2 == 0 && hidden_states.numel() % dim == 0,
                "swiglu_oai: hidden_states must be contiguous with a multiple of dim elements");
    const int64_t rows = hidden_states.numel() / dim;
    at::Tensor out = at::empty({rows, dim / 2}, hidden_states.options());
    const int rc = mi_swiglu_oai(hidden_states.data_ptr(), rows, (int)dim, (float)gemm1_alpha, (float)gemm1_clamp_limit, dtype_code3(hidden_states),
                                 out.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_swiglu_oai failed with code ", rc, " (dim / 2 must be a multiple of 8)");
    return out;
}

// activation/swiglu_oai_quant.py:115-211
std::tuple<at::Tensor, at::Tensor> swiglu_oai_quant(const at::Tensor &x, double alpha, double limit, bool need_quant, const std::optional<at::Tensor> &group_list,
                                                    std::optional<int64_t> group_list_type)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(x.dim() >= 1 && x.is_contiguous() && x.size(-1) % 2 == 0, "swiglu_oai_quant: x must be contiguous [..., 2d]");
    const int64_t h = x.size(-1), rows = h ? x.numel() / h : 0;
    if (group_list.has_value()) {
        TORCH_CHECK(group_list_type.has_value() && (*group_list_type == 0 || *group_list_type == 1), "group_list_type must be 0 or 1, got ",
                    group_list_type.value_or(-1));                                              // reference :151-152
        TORCH_CHECK(group_list->scalar_type() == at::kInt || group_list->scalar_type() == at::kLong, "group_list dtype must be torch.int32 or torch.int64");
        TORCH_CHECK(group_list->is_contiguous() && group_list->dim() == 1, "group_list must be a contiguous vector");
    }
    std::vector<int64_t> oshape(x.sizes().begin(), x.sizes().end());
    oshape.back() = h / 2;
    at::Tensor out = at::empty(oshape, x.options().dtype(need_quant ? at::kChar : x.scalar_type()));
    at::Tensor scale = at::empty({rows}, x.options().dtype(at::kFloat));
    const int rc = mi_swiglu_oai_quant(x.data_ptr(), group_list.has_value() ? group_list->data_ptr() : nullptr,
                                       group_list.has_value() && group_list->scalar_type() == at::kLong, group_list.has_value() ? (int)group_list->numel() : 0,
                                       (int)group_list_type.value_or(0), rows, (int)h, (float)alpha, (float)limit, need_quant, dtype_code(x), out.data_ptr(),
                                       scale.data_ptr<float>(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_swiglu_oai_quant failed with code ", rc);
    return {out, scale};
}

// activation/situ.py:165-480 (situ_and_mul, situ_and_mul_quant, situ share this op)
std::tuple<at::Tensor, at::Tensor> situ_and_mul(const at::Tensor &x, const std::optional<at::Tensor> &group_list, std::optional<int64_t> group_list_type,
                                                double beta, std::optional<double> linear_beta, bool need_quant)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(x.dim() >= 1 && x.is_contiguous() && x.size(-1) % 2 == 0, "situ: x must be contiguous [..., 2d]");
    const int64_t h = x.size(-1), rows = h ? x.numel() / h : 0;
    if (group_list.has_value()) {
        TORCH_CHECK(group_list_type.has_value() && (*group_list_type == 0 || *group_list_type == 1), "group_list_type must be 0 or 1");
        TORCH_CHECK(group_list->scalar_type() == at::kInt || group_list->scalar_type() == at::kLong, "group_list dtype must be torch.int32 or torch.int64");
        TORCH_CHECK(group_list->is_contiguous() && group_list->dim() == 1, "group_list must be a contiguous vector");
    }
    std::vector<int64_t> oshape(x.sizes().begin(), x.sizes().end());
    oshape.back() = h / 2;
    at::Tensor out = at::empty(oshape, x.options().dtype(need_quant ? at::kChar : x.scalar_type()));
    at::Tensor scale = at::empty({rows}, x.options().dtype(at::kFloat));
    const int rc = mi_situ_and_mul(x.data_ptr(), group_list.has_value() ? group_list->data_ptr() : nullptr,
                                   group_list.has_value() && group_list->scalar_type() == at::kLong, group_list.has_value() ? (int)group_list->numel() : 0,
                                   (int)group_list_type.value_or(0), rows, (int)h, (float)beta, linear_beta.has_value() ? (float)*linear_beta : 0.f,
                                   need_quant, dtype_code(x), out.data_ptr(), scale.data_ptr<float>(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_situ_and_mul failed with code ", rc);
    return {out, scale};
}

// kimi_k3/attn_residual.py:66-111
at::Tensor attn_residual_mix(const at::Tensor &prefix_sum, const at::Tensor &bank, int64_t num_valid_blocks, const at::Tensor &combined_weight,
                             double variance_epsilon)
{
    const c10::DeviceGuard device_guard(prefix_sum.device());
    TORCH_CHECK(prefix_sum.dim() == 2 && bank.dim() == 3 && prefix_sum.stride(1) == 1 && bank.stride(2) == 1 && bank.size(0) == prefix_sum.size(0) &&
                    bank.size(2) == prefix_sum.size(1) && bank.scalar_type() == prefix_sum.scalar_type(),
                "mix_fused: prefix_sum [tokens, hidden], bank [tokens, blocks, hidden], hidden contiguous, one dtype");
    TORCH_CHECK(combined_weight.numel() == prefix_sum.size(1) && combined_weight.is_contiguous(), "mix_fused: combined_weight [hidden]");
    TORCH_CHECK(num_valid_blocks >= 0 && num_valid_blocks <= 63, "mix_fused: num_valid_blocks must be in [0, 63] in this build (got ", num_valid_blocks, ")");
    // the kernel moves 16-byte vectors: sliced views whose rows do not start on 16 bytes (bank[:, :, 4:], odd row strides) are copied first
    auto vec_ok = [](const at::Tensor &t, std::initializer_list<int64_t> strides) {
        if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) return false;
        for (int64_t st : strides) if ((st * (int64_t)t.element_size()) % 16) return false;
        return true;
    };
    const at::Tensor prefix_sum_c = vec_ok(prefix_sum, {prefix_sum.stride(0)}) ? prefix_sum : prefix_sum.contiguous();
    const at::Tensor bank_c = vec_ok(bank, {bank.stride(0), bank.stride(1)}) ? bank : bank.contiguous();
    const at::Tensor &prefix_sum_ = prefix_sum_c, &bank_ = bank_c;
    at::Tensor out = at::empty_like(prefix_sum, at::MemoryFormat::Contiguous);
    const int rc = mi_attn_residual_mix(prefix_sum_.data_ptr(), prefix_sum_.stride(0), bank_.data_ptr(), bank_.stride(0), bank_.stride(1),
                                        combined_weight.data_ptr(), dtype_code3(combined_weight), prefix_sum.size(0), (int)num_valid_blocks,
                                        (int)prefix_sum.size(1), (float)variance_epsilon, dtype_code(prefix_sum), out.data_ptr(), out.stride(0),
                                        cur_stream());
    TORCH_CHECK(rc == 0, "mi_attn_residual_mix failed with code ", rc, " (hidden % 8 == 0; at most 63 blocks)");
    return out;
}

// moe/mul_add.py:38-60
at::Tensor mul_add(const at::Tensor &routed_input, const at::Tensor &shared_input, double scaling_factor)
{
    const c10::DeviceGuard device_guard(routed_input.device());
    TORCH_CHECK(routed_input.dim() == 2 && routed_input.is_contiguous() && shared_input.is_contiguous() && shared_input.sizes() == routed_input.sizes() &&
                    shared_input.scalar_type() == routed_input.scalar_type(), "mul_add: two contiguous [batch, hidden] tensors of one dtype");
    at::Tensor out = at::empty_like(routed_input);
    const int rc = mi_mul_add(routed_input.data_ptr(), shared_input.data_ptr(), (float)scaling_factor, routed_input.numel(), dtype_code3(routed_input),
                              out.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_mul_add failed with code ", rc);
    return out;
}

// moe/zero_experts_compute_identity.py:50-81 (expert_indices and expert_scales are modified in place)
at::Tensor zero_experts_compute_identity(at::Tensor &expert_indices, at::Tensor &expert_scales, int64_t num_experts, const at::Tensor &hidden_states,
                                         int64_t identity_mask_value)
{
    const c10::DeviceGuard device_guard(hidden_states.device());
    TORCH_CHECK(hidden_states.dim() == 2 && hidden_states.is_contiguous() && expert_indices.dim() == 2 && expert_indices.is_contiguous() &&
                    expert_scales.is_contiguous() && expert_scales.sizes() == expert_indices.sizes() && expert_indices.size(0) == hidden_states.size(0),
                "zero_experts_compute_identity: hidden [S, D], indices / scales [S, K], all contiguous");
    TORCH_CHECK(expert_indices.scalar_type() == at::kInt || expert_indices.scalar_type() == at::kLong, "expert_indices must be int32 or int64");
    TORCH_CHECK(expert_indices.size(1) <= 64, "zero_experts_compute_identity: K <= 64");
    at::Tensor out = at::empty_like(hidden_states);
    const int rc = mi_zero_experts_identity(expert_indices.data_ptr(), expert_indices.scalar_type() == at::kLong, expert_scales.data_ptr(),
                                            dtype_code3(expert_scales), (int)num_experts, hidden_states.data_ptr(), hidden_states.size(0),
                                            (int)expert_indices.size(1), (int)hidden_states.size(1), (int)identity_mask_value, dtype_code(hidden_states),
                                            out.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_zero_experts_identity failed with code ", rc);
    return out;
}

// norm/fused_split_qk_norm.py:93-134 (weights / biases of the two layer norms passed as tensors)
std::tuple<at::Tensor, at::Tensor, at::Tensor> fused_split_qk_norm(const at::Tensor &x, const at::Tensor &q_weight, const std::optional<at::Tensor> &q_bias,
                                                                   const at::Tensor &k_weight, const std::optional<at::Tensor> &k_bias, int64_t q_lora_rank,
                                                                   int64_t kv_lora_rank, int64_t qk_rope_dim, double eps)
{
    const c10::DeviceGuard device_guard(x.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && x.size(1) == q_lora_rank + kv_lora_rank + qk_rope_dim,
                "fused_split_qk_norm: input must be contiguous [B, q_lora_rank + kv_lora_rank + qk_rope_dim]");
    auto chk = [&](const at::Tensor &t, int64_t n, const char *what) {
        TORCH_CHECK(t.numel() == n && t.is_contiguous() && t.scalar_type() == x.scalar_type(), "fused_split_qk_norm: ", what, " must hold ", n,
                    " values in the input dtype");
    };
    chk(q_weight, q_lora_rank, "q weight"), chk(k_weight, kv_lora_rank, "k weight");
    if (q_bias.has_value()) chk(*q_bias, q_lora_rank, "q bias");
    if (k_bias.has_value()) chk(*k_bias, kv_lora_rank, "k bias");
    const int64_t B = x.size(0);
    at::Tensor q = at::empty({B, q_lora_rank}, x.options()), kn = at::empty({B, kv_lora_rank}, x.options()), kp = at::empty({B, qk_rope_dim}, x.options());
    const int rc = mi_fused_split_qk_norm(x.data_ptr(), B, (int)q_lora_rank, (int)kv_lora_rank, (int)qk_rope_dim, (float)eps, q_weight.data_ptr(),
                                          q_bias.has_value() ? q_bias->data_ptr() : nullptr, k_weight.data_ptr(),
                                          k_bias.has_value() ? k_bias->data_ptr() : nullptr, dtype_code3(x), q.data_ptr(), kn.data_ptr(), kp.data_ptr(),
                                          cur_stream());
    TORCH_CHECK(rc == 0, "mi_fused_split_qk_norm failed with code ", rc);
    return {q, kn, kp};
}

// norm/split_qkv_rmsnorm_rope_pos_cache_half_npu.py:232-407
std::tuple<at::Tensor, at::Tensor, at::Tensor> split_qkv_rmsnorm_rope_pos_cache_half(
    const at::Tensor &input, const at::Tensor &positions, const at::Tensor &cos_sin_cache, int64_t q_hidden_size, int64_t kv_hidden_size,
    int64_t head_dim, std::optional<double> eps, const std::optional<at::Tensor> &q_weight, const std::optional<at::Tensor> &k_weight,
    const std::optional<at::Tensor> &q_bias, const std::optional<at::Tensor> &k_bias, int64_t rope_dim, bool cast_norm_to_bf16)
{
    const c10::DeviceGuard device_guard(input.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(input.dim() == 2 && input.is_contiguous() && input.size(1) == q_hidden_size + 2 * kv_hidden_size,
                "split_qkv_rmsnorm_rope_pos_cache_half: input must be contiguous [B, q + 2 kv]");
    const int64_t B = input.size(0);
    TORCH_CHECK(positions.numel() == B && positions.is_contiguous() && (positions.scalar_type() == at::kInt || positions.scalar_type() == at::kLong),
                "positions must be [B], int32 or int64");
    TORCH_CHECK(cos_sin_cache.dim() == 2 && cos_sin_cache.is_contiguous() && cos_sin_cache.size(0) >= 1 && cos_sin_cache.size(1) >= rope_dim,
                "cos_sin_cache must be contiguous [max_seq, rope_dim]");
    TORCH_CHECK((head_dim & (head_dim - 1)) == 0 && head_dim >= 64 && head_dim <= 256 && rope_dim % 16 == 0 && rope_dim <= head_dim,
                "split_qkv_rmsnorm_rope_pos_cache_half: head_dim must be 64, 128 or 256 and rope_dim a multiple of 16 (this build)");
    TORCH_CHECK(q_hidden_size % kv_hidden_size == 0, "q_hidden_size % kv_hidden_size != 0");
    const bool norms = eps.has_value();
    if (norms)
        TORCH_CHECK(q_weight.has_value() && k_weight.has_value() && q_weight->numel() >= head_dim && k_weight->numel() >= head_dim &&
                        q_weight->scalar_type() == input.scalar_type() && k_weight->scalar_type() == input.scalar_type(),
                    "When using RMSNorm (eps is not None), q_weight / k_weight must have at least head_dim elements in the input dtype");
    TORCH_CHECK(q_bias.has_value() == k_bias.has_value(), "q_bias and k_bias go together");
    if (q_bias.has_value())
        TORCH_CHECK(norms && q_bias->numel() >= head_dim && k_bias->numel() >= head_dim && q_bias->scalar_type() == input.scalar_type() &&
                        k_bias->scalar_type() == input.scalar_type(),
                    "bias needs the norm, head_dim elements and the input dtype");
    at::Tensor q = at::empty({B, q_hidden_size}, input.options()), k = at::empty({B, kv_hidden_size}, input.options()),
               v = at::empty({B, kv_hidden_size}, input.options());
    // contiguous copies (no-ops for contiguous arguments) held in locals that outlive the launch
    const at::Tensor qw_c = q_weight.has_value() ? q_weight->contiguous() : at::Tensor(), kw_c = k_weight.has_value() ? k_weight->contiguous() : at::Tensor(),
                     qb_c = q_bias.has_value() ? q_bias->contiguous() : at::Tensor(), kb_c = k_bias.has_value() ? k_bias->contiguous() : at::Tensor();
    auto p = [](const at::Tensor &t) -> const void * { return t.defined() ? t.data_ptr() : nullptr; };
    const int rc = mi_split_qkv_rmsnorm_rope_pos_cache(input.data_ptr(), positions.data_ptr(), positions.scalar_type() == at::kLong, cos_sin_cache.data_ptr(),
                                                       dtype_code3(cos_sin_cache), (int)cos_sin_cache.size(0), cos_sin_cache.stride(0), (int)B,
                                                       (int)q_hidden_size, (int)kv_hidden_size, (int)head_dim, (int)rope_dim, norms, (float)eps.value_or(0.0),
                                                       p(qw_c), p(kw_c), p(qb_c), p(kb_c), cast_norm_to_bf16, dtype_code(input), q.data_ptr(),
                                                       k.data_ptr(), v.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_split_qkv_rmsnorm_rope_pos_cache failed with code ", rc);
    return {q, k, v};
}

// norm/split_qkv_tp_rmsnorm_rope.py:179-288, first launch: (v, qk_var [batch, 2] fp32 = mean(q^2), mean(k^2) of this rank's columns)
std::tuple<at::Tensor, at::Tensor> split_qkv_tp_local_var(const at::Tensor &input, int64_t q_hidden_size, int64_t kv_hidden_size)
{
    const c10::DeviceGuard device_guard(input.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(input.dim() == 2 && input.is_contiguous() && input.size(1) == q_hidden_size + 2 * kv_hidden_size,
                "split_qkv_tp_rmsnorm_rope: input must be contiguous [batch, q + 2 kv]");
    const int64_t B = input.size(0);
    at::Tensor v = at::empty({B, kv_hidden_size}, input.options());
    at::Tensor qk_var = at::empty({B, 2}, input.options().dtype(at::kFloat));
    const int rc = mi_split_qkv_tp_var(input.data_ptr(), B, (int)q_hidden_size, (int)kv_hidden_size, dtype_code3(input), v.data_ptr(),
                                       qk_var.data_ptr<float>(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_split_qkv_tp_var failed with code ", rc);
    return {v, qk_var};
}

// second launch, behind the all-reduce of qk_var: (q, k)
std::tuple<at::Tensor, at::Tensor> split_qkv_tp_norm_rope(const at::Tensor &input, const at::Tensor &cos, const at::Tensor &sin, const at::Tensor &qk_var,
                                                          int64_t q_hidden_size, int64_t kv_hidden_size, int64_t head_dim, double eps,
                                                          const at::Tensor &q_weight, const at::Tensor &k_weight, int64_t rotary_dim, double inv_tp_world)
{
    const c10::DeviceGuard device_guard(input.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(input.dim() == 2 && input.is_contiguous() && input.size(1) == q_hidden_size + 2 * kv_hidden_size,
                "split_qkv_tp_rmsnorm_rope: input must be contiguous [batch, q + 2 kv]");
    const int64_t B = input.size(0);
    TORCH_CHECK((head_dim & (head_dim - 1)) == 0, "head_dim must be a power of two");              // reference :229-230
    TORCH_CHECK(q_hidden_size % kv_hidden_size == 0, "q_hidden_size % kv_hidden_size != 0");         // reference :231
    TORCH_CHECK(cos.numel() == B * rotary_dim && sin.numel() == B * rotary_dim && cos.is_contiguous() && sin.is_contiguous() &&
                    cos.scalar_type() == input.scalar_type() && sin.scalar_type() == input.scalar_type(),
                "split_qkv_tp_rmsnorm_rope: cos / sin must be contiguous [batch, rotary_dim] in the input dtype");
    TORCH_CHECK(q_weight.numel() == q_hidden_size && k_weight.numel() == kv_hidden_size && q_weight.is_contiguous() && k_weight.is_contiguous() &&
                    q_weight.scalar_type() == input.scalar_type() && k_weight.scalar_type() == input.scalar_type(),
                "split_qkv_tp_rmsnorm_rope: weights must be [q_hidden_size] / [kv_hidden_size] in the input dtype");
    TORCH_CHECK(qk_var.numel() == 2 * B && qk_var.is_contiguous() && qk_var.scalar_type() == at::kFloat, "qk_var must be float32 [batch, 2]");
    at::Tensor q = at::empty({B, q_hidden_size}, input.options()), k = at::empty({B, kv_hidden_size}, input.options());
    const int rc = mi_split_qkv_tp_norm_rope(input.data_ptr(), cos.data_ptr(), sin.data_ptr(), qk_var.data_ptr<float>(), B, (int)q_hidden_size,
                                             (int)kv_hidden_size, (int)head_dim, (int)rotary_dim, (float)eps, (float)inv_tp_world, q_weight.data_ptr(),
                                             k_weight.data_ptr(), dtype_code3(input), q.data_ptr(), k.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_split_qkv_tp_norm_rope failed with code ", rc);
    return {q, k};
}

// split [q | gate] + K + V, Gemma RMSNorm + neox RoPE; arguments as split_qkvgate_gemma_rmsnorm_rope (norm/split_qkv_rmsnorm_rope.py:686-745)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> split_qkvgate_gemma_rmsnorm_rope(
    const at::Tensor &input, const at::Tensor &sin, const at::Tensor &cos, int64_t q_hidden_size, int64_t kv_hidden_size,
    int64_t head_dim, int64_t rope_dim, double eps, const at::Tensor &q_weight, const at::Tensor &k_weight)
{
    const c10::DeviceGuard device_guard(input.device());   // launches and the current stream follow the tensor's GPU
    TORCH_CHECK(input.dim() == 2 && input.is_contiguous(), "split_qkvgate_gemma_rmsnorm_rope: input must be contiguous [batch, 2q+2kv]");
    TORCH_CHECK((head_dim & (head_dim - 1)) == 0, "head_dim must be a power of two");        // reference :700-701
    TORCH_CHECK(q_hidden_size % kv_hidden_size == 0, "q_hidden_size % kv_hidden_size != 0");   // reference :702
    TORCH_CHECK(input.size(1) == 2 * q_hidden_size + 2 * kv_hidden_size, "split_qkvgate_gemma_rmsnorm_rope: input width");
    const int64_t B = input.size(0);
    TORCH_CHECK(sin.numel() == B * rope_dim && cos.numel() == B * rope_dim && sin.is_contiguous() && cos.is_contiguous() &&
                    sin.scalar_type() == input.scalar_type() && cos.scalar_type() == input.scalar_type(),
                "split_qkvgate_gemma_rmsnorm_rope: sin/cos must be contiguous [batch, ..., rope_dim] in the input dtype");
    TORCH_CHECK(q_weight.numel() == head_dim && k_weight.numel() == head_dim && q_weight.is_contiguous() && k_weight.is_contiguous() &&
                    q_weight.scalar_type() == input.scalar_type() && k_weight.scalar_type() == input.scalar_type(),
                "split_qkvgate_gemma_rmsnorm_rope: norm weights must be [head_dim] in the input dtype");
    at::Tensor q = at::empty({B, q_hidden_size}, input.options()), k = at::empty({B, kv_hidden_size}, input.options()),
               v = at::empty({B, kv_hidden_size}, input.options()), gate = at::empty({B, q_hidden_size}, input.options());
    const int rc = mi_split_qkvgate_gemma_rmsnorm_rope(input.data_ptr(), sin.data_ptr(), cos.data_ptr(), (int)B, (int)q_hidden_size,
                                                       (int)kv_hidden_size, (int)head_dim, (int)rope_dim, (float)eps, q_weight.data_ptr(),
                                                       k_weight.data_ptr(), dtype_code(input), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                                       gate.data_ptr(), cur_stream());
    TORCH_CHECK(rc == 0, "mi_split_qkvgate_gemma_rmsnorm_rope failed with code ", rc);
    return {q, k, v, gate};
}

// torch.ops.npu.mla_preprocess: same schema as the reference (csrc/pytorch_extensions.cpp:105-115; host
// csrc/mla_preprocess/op_host/mla_preprocess.cpp:623-704).  MI355X layouts: wdqkv int8 [2112, hidden] and wuq int8
// [q_heads*192, 1536] are plain row-major (output channel major, K contiguous) instead of the Ascend NZ fractal format;
// wuk [q_heads, 128, 512]; kv_cache [blocks, block_size, 1, 512] + kv_cache_rope [blocks, block_size, 1, 64]
// (cache_mode "krope_ctkv": [slot][dim]; "nzcache": per block [dim/16][slot in block][16]; "int8_nzcache": k_nope quantised with
// ctkv_scale into [dim/32][slot in block][32] and q_out0 as int8 quantised with q_nope_scale[head] -- the cache block is the
// unit of the NZ layouts, weights stay row-major).  gamma0 / beta0 are accepted and unused, as in the reference's bf16 kernel (stage 1 is
// quant-only).  Every stage is a HIP kernel of csrc/kernels/mla_gemm.hip (the two INT8 GEMMs and the per-head BMM, hand-written
// skinny split-K / weight-streaming kernels) or csrc/kernels/mla_preprocess.hip (quant, dequant + split + RMSNorm + RoPE + cache).
// wuk is consumed K-contiguous: its [q_heads, 512, 128] transpose is made once per weight tensor and kept (the reference casts
// its weights to the NZ format once as well).
static at::Tensor prepared_wuk(const at::Tensor &wuk, at::ScalarType dtype)
{
    // Keyed on the CALLER's tensor (address, version, target dtype): a dtype conversion happens inside the make step, so a wuk
    // stored in another dtype than the activations still hits.  Inference tensors carry no version counter (_version() throws):
    // they are recorded as version -1 and matched on (address, held storage, shape, dtype) alone.
    struct Entry {
        at::Tensor src, t;      // the source is held: its storage cannot be recycled for another weight while the entry lives
        int64_t version;
    };
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, Entry> cache;
    const int64_t ver = wuk.is_inference() ? -1 : (int64_t)wuk._version();
    const auto key = std::make_pair((const void *)wuk.data_ptr(), (int)dtype);
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end() && it->second.version == ver && it->second.src.sizes() == wuk.sizes() &&
        it->second.src.scalar_type() == wuk.scalar_type())
        return it->second.t;
    if (cache.size() >= 256) cache.clear();
    at::Tensor t = wuk.to(dtype).transpose(1, 2).contiguous();
    cache[key] = Entry{wuk, t, ver};
    return t;
}

std::tuple<at::Tensor &, at::Tensor &, at::Tensor &, at::Tensor &> mla_preprocess(
    const at::Tensor &hiddenState, const at::Tensor &gamma0, const at::Tensor &beta0, const at::Tensor &wdqkv,
    const at::Tensor &descale0, const at::Tensor &gamma1, const at::Tensor &beta1, const at::Tensor &wuq,
    const at::Tensor &descale1, const at::Tensor &gamma2, const at::Tensor &cos, const at::Tensor &sin, const at::Tensor &wuk,
    const at::Tensor &kv_cache, const at::Tensor &kv_cache_rope, const at::Tensor &slotmapping, const at::Tensor &quant_scale0,
    const at::Tensor &quant_offset0, const at::Tensor &bias0, const at::Tensor &quant_scale1, const at::Tensor &quant_offset1,
    const at::Tensor &bias1, const std::optional<at::Tensor> &ctkv_scale, const std::optional<at::Tensor> &q_nope_scale,
    std::optional<c10::string_view> cache_mode, std::optional<c10::string_view> quant_mode, at::Tensor &q_out0,
    at::Tensor &kv_cache_out0, at::Tensor &q_out1, at::Tensor &kv_cache_out1)
{
    const c10::DeviceGuard device_guard(hiddenState.device());   // launches and the current stream follow the tensor's GPU
    (void)gamma0, (void)beta0;
    // cache_mode (csrc/mla_preprocess/op_host/mla_preprocess.cpp:605-606,634): krope_ctkv = 1 (default), int8_nzcache = 2, nzcache = 3
    const c10::string_view cmode = cache_mode.value_or("krope_ctkv");
    TORCH_CHECK(cmode == "krope_ctkv" || cmode == "int8_nzcache" || cmode == "nzcache", "Unsupported cache_mode value: '", cmode, "'");
    const int cmode_i = cmode == "krope_ctkv" ? 1 : cmode == "int8_nzcache" ? 2 : 3;
    // quant_mode: "per_tensor_quant_asymm" (the mode the reference tests cover) or "per_token_quant_symm" -- the reference's DEFAULT
    // when the argument is omitted (csrc/mla_preprocess/op_host/mla_preprocess.cpp:634-635), so it is the default here too
    const c10::string_view qmode = quant_mode.value_or("per_token_quant_symm");
    TORCH_CHECK(qmode == "per_tensor_quant_asymm" || qmode == "per_token_quant_symm", "Unsupported quant_mode value: '", qmode, "'");
    const bool per_token = qmode == "per_token_quant_symm";
    TORCH_CHECK(hiddenState.dim() == 2 && hiddenState.is_contiguous(), "hiddenState must be contiguous [tokens, hidden]");
    const int64_t N = hiddenState.size(0), hidden = hiddenState.size(1);
    TORCH_CHECK(N <= 1024, "mla_preprocess: tokenNum <= 1024 (csrc/mla_preprocess/README.md)");
    TORCH_CHECK(wdqkv.scalar_type() == at::kChar && wdqkv.dim() == 2 && wdqkv.size(0) == 2112 && wdqkv.size(1) == hidden &&
                    wdqkv.is_contiguous(), "wdqkv must be int8 [2112, hidden] row-major");
    TORCH_CHECK(wuq.scalar_type() == at::kChar && wuq.dim() == 2 && wuq.size(1) == 1536 && wuq.size(0) % 192 == 0 && wuq.is_contiguous(),
                "wuq must be int8 [q_heads*192, 1536] row-major");
    const int64_t Hq = wuq.size(0) / 192;
    TORCH_CHECK(wuk.dim() == 3 && wuk.size(0) == Hq && wuk.size(1) == 128 && wuk.size(2) == 512, "wuk must be [q_heads, 128, 512]");
    TORCH_CHECK(descale0.scalar_type() == at::kFloat && descale0.numel() == 2112 && descale1.scalar_type() == at::kFloat &&
                    descale1.numel() == Hq * 192, "descale0 / descale1 must be float32 [2112] / [q_heads*192]");
    TORCH_CHECK(slotmapping.scalar_type() == at::kInt && slotmapping.numel() == N, "slotmapping must be int32 [tokens]");
    TORCH_CHECK(cos.numel() == N * 64 && sin.numel() == N * 64 && cos.is_contiguous() && sin.is_contiguous(), "cos / sin must be [tokens, 64]");
    TORCH_CHECK(kv_cache.is_contiguous() && kv_cache.size(-1) == 512 && kv_cache_rope.is_contiguous() && kv_cache_rope.size(-1) == 64,
                "kv_cache [..., 512] and kv_cache_rope [..., 64] must be contiguous");
    TORCH_CHECK(q_out0.is_contiguous() && q_out0.numel() == N * Hq * 512 && q_out1.is_contiguous() && q_out1.numel() == N * Hq * 64,
                "q_out0 [tokens, q_heads, 512] / q_out1 [tokens, q_heads, 64]");
    int64_t block_size = 0;
    if (cmode_i != 1) {        // the NZ layouts are defined per cache block: [blocks, block_size, 1, dim]
        TORCH_CHECK(kv_cache.dim() >= 2 && kv_cache_rope.dim() == kv_cache.dim() && kv_cache_rope.size(1) == kv_cache.size(1),
                    "nzcache modes need kv_cache [blocks, block_size, ..., 512] and kv_cache_rope with the same block_size");
        block_size = kv_cache.size(1);
    }
    if (cmode_i == 2) {
        TORCH_CHECK(kv_cache.scalar_type() == at::kChar && q_out0.scalar_type() == at::kChar,
                    "cache_mode='int8_nzcache': kv_cache and q_out0 must be int8");
        TORCH_CHECK(ctkv_scale.has_value() && ctkv_scale->numel() == 1 && ctkv_scale->scalar_type() == hiddenState.scalar_type() &&
                        q_nope_scale.has_value() && q_nope_scale->numel() == Hq && q_nope_scale->is_contiguous() &&
                        q_nope_scale->scalar_type() == hiddenState.scalar_type(),
                    "cache_mode='int8_nzcache' needs ctkv_scale [1] and q_nope_scale [q_heads] in the input dtype");
    } else {
        TORCH_CHECK(kv_cache.scalar_type() == hiddenState.scalar_type() && q_out0.scalar_type() == hiddenState.scalar_type(),
                    "kv_cache / q_out0 must have the input dtype");
    }
    TORCH_CHECK(kv_cache_rope.scalar_type() == hiddenState.scalar_type() && q_out1.scalar_type() == hiddenState.scalar_type(),
                "kv_cache_rope / q_out1 must have the input dtype");
    const int dt = dtype_code(hiddenState);
    auto dev = hiddenState.device();
    void *st = cur_stream();
    TORCH_CHECK(per_token ||
                    (quant_scale0.numel() == 1 && quant_scale1.numel() == 1 && quant_scale0.scalar_type() == hiddenState.scalar_type() &&
                     quant_scale1.scalar_type() == hiddenState.scalar_type() && quant_offset0.numel() == 1 && quant_offset1.numel() == 1 &&
                     quant_offset0.scalar_type() == at::kChar && quant_offset1.scalar_type() == at::kChar),
                "quant_scale0/1 must be [1] in the input dtype, quant_offset0/1 int8 [1]");
    // five launches on the caller's stream, no library GEMM (stage order of mla_preprocess_mix_bf16.hpp):
    //   quant -> INT8 GEMM1 split-K (partial products) -> sum + dequant / RMSNorm / RoPE / cache write / requant
    //   -> INT8 GEMM2 with the dequant epilogue -> per-head BMM + RoPE of the positional columns
    auto i8 = at::dtype(at::kChar).device(dev);
    at::Tensor a8 = at::empty({N, hidden}, i8);
    const int parts = mi_mla_pre_gemm_i8_partials((int)hidden);                 // split-K partial products, summed by pre_mid
    at::Tensor c1 = at::empty({parts, N, 2112}, at::dtype(at::kInt).device(dev));
    // per-token mode: every row is quantised against its own maximum and carries its scale to the dequant of the following GEMM
    at::Tensor tok0, tok1;
    if (per_token) tok0 = at::empty({N}, at::dtype(at::kFloat).device(dev)), tok1 = at::empty({N}, at::dtype(at::kFloat).device(dev));
    at::Tensor q8 = at::empty({N, 1536}, i8);
    auto iptr = [](const at::Tensor &t) -> const int32_t * { return t.numel() ? t.data_ptr<int32_t>() : nullptr; };
    // Opt-in (MI_MLA_PRE_ONE_LAUNCH=1), decode sizes: the whole op as ONE launch (stage bodies of the four launches behind grid barriers
    // inside one grid; bit-identical; measured no faster than the four launches, csrc/kernels/mla_gemm.hip).  The barrier words come
    // from a per-device ring: a buffer serves one call in flight, calls on different streams get different buffers.
    const char *ol_env = getenv("MI_MLA_PRE_ONE_LAUNCH");      // read per call: the tests compare both forms in one process
    const bool one_launch = ol_env && atoi(ol_env) != 0;
    if (one_launch && N > 0) {
        constexpr int kRing = 16;
        static std::mutex mu;
        // (never destroyed: a static tensor freed at process exit would outlive the HIP context)
        static auto &rings = *new std::map<int, std::pair<at::Tensor, uint64_t>>();
        const int64_t words = (int64_t)mi_mla_preprocess_one_launch_sync_words();
        uint32_t *sync = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu);
            auto &r = rings[dev.index()];
            if (!r.first.defined()) r.first = at::zeros({kRing, words}, at::dtype(at::kInt).device(dev));
            sync = (uint32_t *)r.first.data_ptr<int32_t>() + (r.second++ % kRing) * words;
        }
        at::Tensor wuk_t1 = prepared_wuk(wuk, hiddenState.scalar_type());
        const int rc = mi_mla_preprocess_one_launch(
            hiddenState.data_ptr(), (int)N, (int)hidden, per_token ? nullptr : quant_scale0.data_ptr(),
            per_token ? nullptr : (const int8_t *)quant_offset0.data_ptr(), (int8_t *)a8.data_ptr(), per_token ? tok0.data_ptr<float>() : nullptr,
            (const int8_t *)wdqkv.data_ptr(), c1.data_ptr<int32_t>(), iptr(bias0), descale0.data_ptr<float>(), gamma1.data_ptr(), beta1.data_ptr(),
            gamma2.data_ptr(), cos.data_ptr(), sin.data_ptr(), slotmapping.data_ptr<int32_t>(), per_token ? nullptr : quant_scale1.data_ptr(),
            per_token ? nullptr : (const int8_t *)quant_offset1.data_ptr(), 1e-6f, (int8_t *)q8.data_ptr(), kv_cache.data_ptr(),
            kv_cache_rope.data_ptr(), per_token ? tok1.data_ptr<float>() : nullptr, cmode_i, (int)block_size,
            cmode_i == 2 ? ctkv_scale->data_ptr() : nullptr, (const int8_t *)wuq.data_ptr(), (int)Hq, per_token ? nullptr : iptr(bias1),
            descale1.data_ptr<float>(), wuk_t1.data_ptr(), q_out0.data_ptr(), q_out1.data_ptr(), cmode_i == 2 ? q_nope_scale->data_ptr() : nullptr,
            per_token ? 1 : 0, dt, sync, st);
        TORCH_CHECK(rc == 0 || rc == MI_SGL_ENOTAPPLICABLE, "mi_mla_preprocess_one_launch failed with code ", rc);
        if (rc == 0) {
            if (kv_cache_out0.data_ptr() != kv_cache.data_ptr()) kv_cache_out0.copy_(kv_cache);
            if (kv_cache_out1.data_ptr() != kv_cache_rope.data_ptr()) kv_cache_out1.copy_(kv_cache_rope);
            return {q_out0, kv_cache_out0, q_out1, kv_cache_out1};
        }
    }
    if (per_token) {
        TORCH_CHECK(0 == mi_mla_pre_quant_token(hiddenState.data_ptr(), (int)N, (int)hidden, dt, (int8_t *)a8.data_ptr(), tok0.data_ptr<float>(), st),
                    "mi_mla_pre_quant_token failed");
    } else {
        TORCH_CHECK(0 == mi_mla_pre_quant(hiddenState.data_ptr(), quant_scale0.data_ptr(), (const int8_t *)quant_offset0.data_ptr(), N * hidden, dt,
                                          (int8_t *)a8.data_ptr(), st), "mi_mla_pre_quant failed");
    }
    TORCH_CHECK(0 == mi_mla_pre_gemm_i8((const int8_t *)a8.data_ptr(), (int)N, (int)hidden, (const int8_t *)wdqkv.data_ptr(), 2112, 0,
                                        c1.data_ptr<int32_t>(), nullptr, nullptr, nullptr, nullptr, dt, st), "mi_mla_pre_gemm_i8 (GEMM1) failed");
    TORCH_CHECK(0 == mi_mla_pre_mid(c1.data_ptr<int32_t>(), parts, iptr(bias0), descale0.data_ptr<float>(), gamma1.data_ptr(), beta1.data_ptr(),
                                    gamma2.data_ptr(), cos.data_ptr(), sin.data_ptr(), slotmapping.data_ptr<int32_t>(),
                                    per_token ? nullptr : quant_scale1.data_ptr(), per_token ? nullptr : (const int8_t *)quant_offset1.data_ptr(),
                                    1e-6f, (int)N, dt, (int8_t *)q8.data_ptr(), kv_cache.data_ptr(), kv_cache_rope.data_ptr(),
                                    per_token ? tok0.data_ptr<float>() : nullptr, per_token ? tok1.data_ptr<float>() : nullptr, cmode_i,
                                    (int)block_size, cmode_i == 2 ? ctkv_scale->data_ptr() : nullptr, st),
                "mi_mla_pre_mid failed");
    at::Tensor wuk_t = prepared_wuk(wuk, hiddenState.scalar_type());
    const void *qns = cmode_i == 2 ? q_nope_scale->data_ptr() : nullptr;
    // GEMM2 + per-head BMM + RoPE: one launch, a workgroup per head, the GEMM2 output stays in LDS (MI_MLA_PRE_FUSED=0: the two-launch
    // form with the GEMM2 output materialised in global memory; bit-identical)
    static const bool fused = !(getenv("MI_MLA_PRE_FUSED") && atoi(getenv("MI_MLA_PRE_FUSED")) == 0);
    if (fused) {
        TORCH_CHECK(0 == mi_mla_pre_gemm2_bmm_rope((const int8_t *)q8.data_ptr(), (int)N, (const int8_t *)wuq.data_ptr(), (int)Hq,
                                                   per_token ? nullptr : iptr(bias1), descale1.data_ptr<float>(),
                                                   per_token ? tok1.data_ptr<float>() : nullptr, wuk_t.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                   dt, q_out0.data_ptr(), q_out1.data_ptr(), qns, st), "mi_mla_pre_gemm2_bmm_rope failed");
    } else {
        at::Tensor y2 = at::empty({N, Hq * 192}, hiddenState.options());          // GEMM2 output in the I/O dtype (golden :95-107)
        TORCH_CHECK(0 == mi_mla_pre_gemm_i8((const int8_t *)q8.data_ptr(), (int)N, 1536, (const int8_t *)wuq.data_ptr(), (int)(Hq * 192), 1,
                                            nullptr, per_token ? nullptr : iptr(bias1), descale1.data_ptr<float>(),
                                            per_token ? tok1.data_ptr<float>() : nullptr, y2.data_ptr(), dt, st), "mi_mla_pre_gemm_i8 (GEMM2) failed");
        TORCH_CHECK(0 == mi_mla_pre_bmm_rope(y2.data_ptr(), (int)N, (int)Hq, wuk_t.data_ptr(), cos.data_ptr(), sin.data_ptr(), dt,
                                             q_out0.data_ptr(), q_out1.data_ptr(), qns, st), "mi_mla_pre_bmm_rope failed");
    }
    if (kv_cache_out0.data_ptr() != kv_cache.data_ptr()) kv_cache_out0.copy_(kv_cache);
    if (kv_cache_out1.data_ptr() != kv_cache_rope.data_ptr()) kv_cache_out1.copy_(kv_cache_rope);
    return {q_out0, kv_cache_out0, q_out1, kv_cache_out1};
}

}  // namespace npu_kernel
}  // namespace sglang

TORCH_LIBRARY_FRAGMENT(npu, m)
{
    m.def("sgl_kernel_npu_version() -> str", &sglang::npu_kernel::sgl_kernel_npu_version);
    m.def("decode_mla(Tensor q, Tensor k_nope_buffer, Tensor k_rope_buffer, Tensor(a!) att_out, Tensor kv_seq_lens, "
          "float sm_scale, int page_size, Tensor block_table, int num_splits=0) -> ()");
    m.def("decode_mla_plan(Tensor kv_seq_lens, int num_kv_heads=1) -> Tensor");
    m.def("clear_mla_plan_cache", &sglang::npu_kernel::clear_mla_plan_cache);      // no tensor arguments: catch-all kernel
    m.def("decode_mla_planned(Tensor q, Tensor k_nope_buffer, Tensor k_rope_buffer, Tensor(a!) att_out, Tensor kv_seq_lens, "
          "float sm_scale, int page_size, Tensor block_table, Tensor plan) -> ()");
    m.def("decode_gqa(Tensor q, Tensor k_buffer, Tensor v_buffer, Tensor(a!) att_out, Tensor kv_seq_lens, "
          "float sm_scale, int page_size, Tensor block_table, int num_splits=0) -> ()");
    m.def("mla_preprocess(Tensor hiddenState, Tensor gamma0, Tensor beta0, Tensor wdqkv, "
          "Tensor descale0, Tensor gamma1, Tensor beta1, Tensor wuq, "
          "Tensor descale1, Tensor gamma2, Tensor cos, Tensor sin, Tensor wuk,"
          "Tensor kv_cache, Tensor kv_cache_rope, Tensor slotmapping, "
          "Tensor quant_scale0, Tensor quant_offset0, Tensor bias0, "
          "Tensor quant_scale1, Tensor quant_offset1, Tensor bias1, *, "
          "Tensor? ctkv_scale=None, Tensor? q_nope_scale=None, "
          "str? cache_mode=None, str? quant_mode=None, "
          "Tensor(a!) q_out0, Tensor(b!) kv_cache_out0, Tensor(c!) q_out1, Tensor(d!) kv_cache_out1) "
          "-> (Tensor(a!), Tensor(b!), Tensor(c!), Tensor(d!))");
    m.def("swiglu_quant(Tensor x, Tensor group_list, int group_list_type, bool need_quant=True, bool do_limit=False, "
          "float limit=7.0) -> (Tensor, Tensor)");
    m.def("add_rmsnorm_bias(Tensor input, Tensor? residual, Tensor norm_weight, Tensor? norm_bias, float eps, "
          "Tensor? quant_scale=None, Tensor? quant_offset=None, bool gemma=False) -> (Tensor, Tensor)");
    m.def("fused_rope_qk_mqa(Tensor query, Tensor key, Tensor cos_sin, int rotary_dim, bool is_neox_style) -> (Tensor, Tensor)");
    m.def("split_qkv_rmsnorm_rope(Tensor input, Tensor sin, Tensor cos, int q_hidden_size, int kv_hidden_size, int head_dim, "
          "float? eps=None, Tensor? q_weight=None, Tensor? k_weight=None, Tensor? q_bias=None, Tensor? k_bias=None, "
          "bool is_neox_style=True) -> (Tensor, Tensor, Tensor)");
    m.def("l1_norm(Tensor input) -> Tensor");
    m.def("rmsnorm_without_weight(Tensor x, float eps) -> Tensor");
    m.def("fused_variance(Tensor x) -> Tensor");
    m.def("fused_rsqrt_mul(Tensor x, Tensor variance, Tensor weight, float eps=1e-6) -> Tensor");
    m.def("fused_scale_shift(Tensor x, Tensor scale, Tensor shift, float scale_constant=1.0) -> Tensor");
    m.def("split_qkv_rmsnorm_mrope(Tensor qkv, Tensor q_weight, Tensor k_weight, Tensor cos_sin, int num_q_heads, int num_kv_heads, int head_size, "
          "float eps, int[] mrope_section, bool is_interleaved, int? rope_dim=None, Tensor? q_bias=None, Tensor? k_bias=None, "
          "bool has_gate=False) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("split_qkv_rmsnorm_rope_pos_cache_half(Tensor input, Tensor positions, Tensor cos_sin_cache, int q_hidden_size, int kv_hidden_size, "
          "int head_dim, float? eps, Tensor? q_weight, Tensor? k_weight, Tensor? q_bias, Tensor? k_bias, int rope_dim, "
          "bool cast_norm_to_bf16) -> (Tensor, Tensor, Tensor)");
    m.def("attention_sinks(Tensor query, Tensor k_cache, Tensor v_cache, Tensor sinks, Tensor block_tables, Tensor kv_lens, float scale, "
          "int sliding_window_size, int q_head_num, int k_head_num, Tensor? bt_rows=None) -> Tensor");
    m.def("swiglu_oai_quant(Tensor x, float alpha, float limit, bool need_quant=True, Tensor? group_list=None, int? group_list_type=None) -> (Tensor, Tensor)");
    m.def("situ_and_mul(Tensor x, Tensor? group_list, int? group_list_type, float beta, float? linear_beta, bool need_quant) -> (Tensor, Tensor)");
    m.def("fia_blockq_sparse_prefill(Tensor q, Tensor k_cache, Tensor v_cache, Tensor topk_idx, Tensor seq_lens, Tensor per_query_req, "
          "Tensor req_to_token, int block_size, float sm_scale, Tensor? block_table_out=None, Tensor? actual_kvlen_out=None) -> Tensor");
    m.def("gqa_share_sparse_num_chunks", &sglang::npu_kernel::gqa_share_sparse_num_chunks);      // no tensor arguments: catch-all kernel
    m.def("gqa_share_sparse_decode(Tensor q, Tensor? sink, Tensor k_cache, Tensor v_cache, Tensor? block_table, Tensor seq_lens, Tensor topk_idx, "
          "float sm_scale, int num_chunks=0, Tensor? req_to_token=None, Tensor? req_pool_indices=None, int max_num_blocks=0, int num_pages=0, "
          "bool sanitize_page_ids=False) -> Tensor");
    m.def("gqa_block_score_topk(Tensor q, Tensor k_cache, Tensor? block_table, Tensor seq_lens, int max_seqlen, int topk, int init_blocks, "
          "int local_blocks, float sm_scale, bool score_lse=False, Tensor? req_to_token=None, Tensor? req_pool_indices=None, int max_num_blocks=0, "
          "int num_pages=0, bool sanitize_page_ids=False, bool packed_seq_lens=False, bool append_local=False) -> Tensor");
    m.def("topk_append_local_block(Tensor topk_idx, Tensor seq_lens, int block_size, int num_blocks) -> Tensor");
    m.def("gqa_prefill_block_score(Tensor q, Tensor k_cache, Tensor cu_seqlens, Tensor seq_lens, Tensor req_to_token, Tensor req_pool_indices, "
          "int max_seqlen, float sm_scale, bool lse, Tensor? query_pos=None) -> Tensor");
    m.def("prefill_topk_from_score(Tensor score, Tensor? per_query_seq_lens, int topk, int block_size, bool fused) -> Tensor");
    m.def(
        "lightning_indexer(Tensor query, Tensor key, Tensor weights, Tensor? actual_seq_lengths_query=None, "
        "Tensor? actual_seq_lengths_key=None, Tensor? block_table=None, "
        "str? layout_query=None, str? layout_key=None, "
        "int? sparse_count=None, int? sparse_mode=None) -> Tensor");
    m.def(
        "sparse_attn_sharedkv(Tensor q, *, Tensor? ori_kv=None, Tensor? cmp_kv=None, "
        "Tensor? ori_sparse_indices=None, Tensor? cmp_sparse_indices=None, "
        "Tensor? ori_block_table=None, Tensor? cmp_block_table=None, "
        "Tensor? cu_seqlens_q=None, Tensor? cu_seqlens_ori_kv=None, "
        "Tensor? cu_seqlens_cmp_kv=None, Tensor? seqused_q=None, Tensor? seqused_kv=None, "
        "Tensor? sinks=None, Tensor? metadata=None, float softmax_scale=0, int cmp_ratio=0, "
        "int ori_mask_mode=4, int cmp_mask_mode=3, int ori_win_left=128, int ori_win_right=0, "
        "str layout_q='BSND', str layout_kv='PA_ND', "
        "bool return_softmax_lse=False) -> (Tensor, Tensor)");
    m.def(
        "npu_sparse_attention_score(Tensor query, Tensor key, Tensor value, Tensor select_idx, "
        "Tensor block_table, Tensor? select_num_idx=None, Tensor? q_dequant_scale=None, "
        "Tensor? k_dequant_scale=None, Tensor? v_dequant_scale=None, "
        "Tensor? actual_seq_lengths=None, Tensor? actual_seq_lengths_kv=None, "
        "int num_key_value_heads=1, float scale_value=1.0, int block_size=128, "
        "int top_k=16, int inner_precise=0) -> Tensor");
    m.def(
        "compressor(Tensor x, Tensor wkv, Tensor wgate, Tensor! state_cache, "
        "Tensor ape, Tensor norm_weight, Tensor rope_sin, Tensor rope_cos, "
        "Tensor? state_block_table=None, Tensor? cu_seqlens=None, Tensor? seqused=None, "
        "Tensor? start_pos=None, int rope_head_dim=64, int cmp_ratio=4, int coff=1, "
        "float norm_eps=1e-6, int rotary_mode=1, int cache_mode=1, "
        "int state_cache_stride_dim0=0) -> Tensor");
    m.def("attn_residual_mix(Tensor prefix_sum, Tensor bank, int num_valid_blocks, Tensor combined_weight, float variance_epsilon) -> Tensor");
    m.def("mul_add(Tensor routed_input, Tensor shared_input, float scaling_factor) -> Tensor");
    m.def("zero_experts_compute_identity(Tensor(a!) expert_indices, Tensor(b!) expert_scales, int num_experts, Tensor hidden_states, "
          "int identity_mask_value=0) -> Tensor");
    m.def("swiglu_oai(Tensor hidden_states, int dim, float gemm1_alpha, float gemm1_clamp_limit) -> Tensor");
    m.def("fused_split_qk_norm(Tensor x, Tensor q_weight, Tensor? q_bias, Tensor k_weight, Tensor? k_bias, int q_lora_rank, int kv_lora_rank, "
          "int qk_rope_dim, float eps=1e-6) -> (Tensor, Tensor, Tensor)");
    m.def("split_qkv_tp_local_var(Tensor input, int q_hidden_size, int kv_hidden_size) -> (Tensor, Tensor)");
    m.def("split_qkv_tp_norm_rope(Tensor input, Tensor cos, Tensor sin, Tensor qk_var, int q_hidden_size, int kv_hidden_size, int head_dim, "
          "float eps, Tensor q_weight, Tensor k_weight, int rotary_dim, float inv_tp_world) -> (Tensor, Tensor)");
    m.def("split_qkvgate_gemma_rmsnorm_rope(Tensor input, Tensor sin, Tensor cos, int q_hidden_size, int kv_hidden_size, int head_dim, "
          "int rope_dim, float eps, Tensor q_weight, Tensor k_weight) -> (Tensor, Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(npu, CUDA, m)
{
    m.impl("decode_mla", TORCH_FN(sglang::npu_kernel::decode_mla));
    m.impl("decode_mla_plan", TORCH_FN(sglang::npu_kernel::decode_mla_plan));
    m.impl("decode_mla_planned", TORCH_FN(sglang::npu_kernel::decode_mla_planned));
    m.impl("decode_gqa", TORCH_FN(sglang::npu_kernel::decode_gqa));
    m.impl("mla_preprocess", TORCH_FN(sglang::npu_kernel::mla_preprocess));
    m.impl("swiglu_quant", TORCH_FN(sglang::npu_kernel::swiglu_quant));
    m.impl("add_rmsnorm_bias", TORCH_FN(sglang::npu_kernel::add_rmsnorm_bias));
    m.impl("fused_rope_qk_mqa", TORCH_FN(sglang::npu_kernel::fused_rope_qk_mqa));
    m.impl("split_qkv_rmsnorm_rope", TORCH_FN(sglang::npu_kernel::split_qkv_rmsnorm_rope));
    m.impl("split_qkvgate_gemma_rmsnorm_rope", TORCH_FN(sglang::npu_kernel::split_qkvgate_gemma_rmsnorm_rope));
    m.impl("l1_norm", TORCH_FN(sglang::npu_kernel::l1_norm));
    m.impl("rmsnorm_without_weight", TORCH_FN(sglang::npu_kernel::rmsnorm_without_weight));
    m.impl("fused_variance", TORCH_FN(sglang::npu_kernel::fused_variance));
    m.impl("fused_rsqrt_mul", TORCH_FN(sglang::npu_kernel::fused_rsqrt_mul));
    m.impl("fused_scale_shift", TORCH_FN(sglang::npu_kernel::fused_scale_shift));
    m.impl("split_qkv_rmsnorm_mrope", TORCH_FN(sglang::npu_kernel::split_qkv_rmsnorm_mrope));
    m.impl("split_qkv_rmsnorm_rope_pos_cache_half", TORCH_FN(sglang::npu_kernel::split_qkv_rmsnorm_rope_pos_cache_half));
    m.impl("attention_sinks", TORCH_FN(sglang::npu_kernel::attention_sinks));
    m.impl("swiglu_oai_quant", TORCH_FN(sglang::npu_kernel::swiglu_oai_quant));
    m.impl("situ_and_mul", TORCH_FN(sglang::npu_kernel::situ_and_mul));
    m.impl("fia_blockq_sparse_prefill", TORCH_FN(sglang::npu_kernel::fia_blockq_sparse_prefill));
    m.impl("gqa_share_sparse_decode", TORCH_FN(sglang::npu_kernel::gqa_share_sparse_decode));
    m.impl("gqa_block_score_topk", TORCH_FN(sglang::npu_kernel::gqa_block_score_topk));
    m.impl("topk_append_local_block", TORCH_FN(sglang::npu_kernel::topk_append_local_block));
    m.impl("gqa_prefill_block_score", TORCH_FN(sglang::npu_kernel::gqa_prefill_block_score));
    m.impl("prefill_topk_from_score", TORCH_FN(sglang::npu_kernel::prefill_topk_from_score));
    m.impl("lightning_indexer", TORCH_FN(sglang::npu_kernel::lightning_indexer));
    m.impl("sparse_attn_sharedkv", TORCH_FN(sglang::npu_kernel::sparse_attn_sharedkv));
    m.impl("compressor", TORCH_FN(sglang::npu_kernel::compressor));
    m.impl("npu_sparse_attention_score", TORCH_FN(sglang::npu_kernel::npu_sparse_attention_score));
    m.impl("attn_residual_mix", TORCH_FN(sglang::npu_kernel::attn_residual_mix));
    m.impl("mul_add", TORCH_FN(sglang::npu_kernel::mul_add));
    m.impl("zero_experts_compute_identity", TORCH_FN(sglang::npu_kernel::zero_experts_compute_identity));
    m.impl("swiglu_oai", TORCH_FN(sglang::npu_kernel::swiglu_oai));
    m.impl("fused_split_qk_norm", TORCH_FN(sglang::npu_kernel::fused_split_qk_norm));
    m.impl("split_qkv_tp_local_var", TORCH_FN(sglang::npu_kernel::split_qkv_tp_local_var));
    m.impl("split_qkv_tp_norm_rope", TORCH_FN(sglang::npu_kernel::split_qkv_tp_norm_rope));
}
