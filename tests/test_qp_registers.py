"""The QP kernel instances that need no scratch memory, held to it (build.device_metadata; no GPU)."""
from concurrent.futures import ThreadPoolExecutor

from legged_mpc_control_amd import build as B

# (source, what the mangled name contains, instances): the lone-wave instances of the LDS Riccati kernel
# (lmpc_lq_kernel<1, *, 1> and <2, *, 1>), the dense interior point, the dual active set and the fused dense + Riccati
# kernel, flat and terrain each.  The two-wave instances <*, *, 2> and the scratch Riccati kernel spill by design
# (DESIGN.md 4, 4d).
NO_SCRATCH = (("lmpc_lq.hip", "lmpc_lq_kernelILi1ELb0ELi1E", 1), ("lmpc_lq.hip", "lmpc_lq_kernelILi1ELb1ELi1E", 1),
              ("lmpc_lq.hip", "lmpc_lq_kernelILi2ELb0ELi1E", 1), ("lmpc_lq.hip", "lmpc_lq_kernelILi2ELb1ELi1E", 1),
              ("lmpc_dense.hip", "lmpc_dense_kernel", 2), ("lmpc_gi.hip", "lmpc_gi_kernel", 2),
              ("lmpc_fused.hip", "lmpc_dense_lq_kernel", 2))


def test_qp_kernels_without_scratch_keep_none():
    """Cross-compiled with the product's flags: private_segment_fixed_size == 0 and vgpr_spill_count == 0.  The kernels
    share their interior-point and certificate steps through lmpc_qp_step.h, where how an argument is passed has moved
    spills ("The QP kernels' shared steps, written once"); a refactor or a compiler upgrade that brings
    spills back changes no result, so only this test would notice."""
    sources = sorted({s for s, _, _ in NO_SCRATCH})
    with ThreadPoolExecutor(len(sources)) as ex:
        metas = dict(zip(sources, ex.map(B.device_metadata, sources)))
    for source, pattern, count in NO_SCRATCH:
        meta = {k: v for k, v in metas[source].items() if pattern in k}
        assert len(meta) == count, (source, pattern, list(metas[source]))
        for name, m in meta.items():
            print(f"{name[:60]}...: {m}")
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
