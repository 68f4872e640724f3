"""Counts the compiler-made stalls of the 3x3 phase loops in the assembly of howl_amd/csrc/res8.hip.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Ihowl_amd/csrc -Iinclude howl_amd/csrc/res8.hip -o res8.s
    python tools/isa_phase_loops.py res8.s

Per bench instance: VGPRs, private segment, MFMAs and how many of them accumulate in place (dst == srcC), s_nop, private-segment
instructions, `vmcnt(0)` within six instructions behind a global store, and `ds_read ; lgkmcnt(0) ; v_mfma` triples (an operand
fetched at zero distance)."""
import re
import sys

WANT = ["bwd_pair_kernelILi1ELi1ELi0", "conv3x3_mfma_kernelILi0ELi1ELi0", "conv3x3_mfma_kernelILi1ELi1ELi0", "wgrad_mfma_kernelILi1ELi0"]

lines = open(sys.argv[1]).read().split("\n")
starts = [(i, l) for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
for want in WANT:
    for k, (i, label) in enumerate(starts):
        if want not in label:
            continue
        j = starts[k + 1][0] if k + 1 < len(starts) else len(lines)
        text = "\n".join(lines[i:j])
        ins = [x.strip() for x in lines[i:j] if x.startswith("\t") and not x.strip().startswith((".", ";"))]
        mfma = [x for x in ins if x.startswith("v_mfma")]
        inplace = 0
        for x in mfma:
            ops = [o.strip() for o in x.split(None, 1)[1].split(",")]
            inplace += ops[0] == ops[3]
        store_wait = 0
        for a, x in enumerate(ins):
            if x.startswith("global_store"):
                for y in ins[a + 1:a + 7]:
                    if y.startswith("global_store"):
                        break
                    if "vmcnt(0)" in y:
                        store_wait += 1
                        break
        zero_dist = sum(1 for a, x in enumerate(ins)
                        if x.startswith("v_mfma") and a >= 2 and "lgkmcnt(0)" in ins[a - 1] and ins[a - 2].startswith("ds_read"))
        vgpr = re.search(r"; NumVgprs: (\d+)", text).group(1)
        private = re.search(r"; ScratchSize: (\d+)", text).group(1)
        print(f"{want}: vgpr={vgpr} private={private} "
              f"mfma={len(mfma)} in_place={inplace} s_nop={sum(x.startswith('s_nop') for x in ins)} "
              f"private_ops={sum(x.startswith('scratch_') for x in ins)} store_then_vmcnt0={store_wait} read_wait0_mfma={zero_dist}")
