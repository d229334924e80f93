"""hipcc -Rpass-analysis=kernel-resource-usage of the device sources -> profiles/r<round>_resource_usage.txt (usage: tools/resource_usage.py <round>; a name
instead of a number, e.g. `windows`, writes profiles/<name>_resource_usage.txt)
(VGPRs, spilled VGPRs, scratch bytes per lane, waves/SIMD, LDS bytes per workgroup, SGPRs and spilled SGPRs of every kernel;
spilled SGPRs live in lanes of a VGPR and come back by v_readlane_b32)."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench

cc = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
out = [f"# {cc[0] if cc else 'hipcc'}; {cc[1] if len(cc) > 1 else ''}",
       f"# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on these sources (kernel source sha {bench.kernel_source_sha()})",
       "# kernel | VGPRs | spilled VGPRs | scratch B/lane | waves/SIMD | LDS B/workgroup | SGPRs | spilled SGPRs"]
for src in ("td_kernels.hip", "td_generic.hip", "td_special.hip", "td_rows.hip", "td_pack.hip", "td_windows.hip", "td_labels.hip", "td_select.hip", "td_offsets.hip", "td_ranges.hip", "td_counts.hip", "td_decode_rows.hip", "td_ngrams.hip", "td_join.hip", "td_minhash.hip", "td_nfc.hip", "td_utf8.hip", "td_textstats.hip"):
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT / 'include'}", "-c",
                        str(ROOT / "tokendagger_amd" / "csrc" / src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    cur = {}
    for line in p.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs|SGPRs Spill|VGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (.*?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}
        cur[k] = v
        if k.startswith("LDS") and "rocprim" not in cur["name"]:  # (td_pack.hip: the library's scan, sort and run-length kernels are not ours)
            name = cur["name"].replace("td::", "").replace("(td::EncodeArgs)", "").replace("(anonymous namespace)::", "").replace("(td::WindowArgs)", "").replace("(td::LabelArgs)", "").replace("(td::RowsArgs)", "").replace("(td::PackArgs)", "").replace("(td::SelectArgs)", "").replace("(td::RangeArgs)", "").replace("(td::CountsArgs)", "").replace("(td::DecodeRowsArgs)", "").replace("(td::DcrMarkArgs)", "").replace("(td::NgramArgs)", "").replace("(td::NgramArgs, long, int)", "").replace("(td::JoinArgs)", "").replace("(td::MhashArgs)", "").replace("(td::NfcArgs)", "").replace("(td::U8Args)", "").replace("(td::TsArgs)", "")
            out.append(f"{name} | {cur['VGPRs']} | {cur['VGPRs Spill']} | {cur['ScratchSize [bytes/lane]']} | {cur['Occupancy [waves/SIMD]']} | {v} | {cur['TotalSGPRs']} | {cur['SGPRs Spill']}")
tag = sys.argv[1] if len(sys.argv) > 1 else "6"
(ROOT / "profiles" / f"{'r' + tag if tag.isdigit() else tag}_resource_usage.txt").write_text("\n".join(out) + "\n")
print("\n".join(out))
