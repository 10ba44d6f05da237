"""The packer of the key-table kernels' auxiliary block (audiowmark_amd/csrc/host/keytab_stage.hh) under the address and
undefined-behaviour sanitizers, on the CPU: tests/keytab_pack_check.cc is built as a stand-alone program from the header and host/aes128.cc
-- plain C++, no HIP runtime -- and run.  It packs 1, 3 and 257 keys, with and without a payload's coded bytes, into heap blocks of
exactly the returned size and checks the S-box, the coded bytes and every key schedule at the returned offsets."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "..", "audiowmark_amd", "csrc", "host")


def test_packer_under_the_sanitizers(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [p for p in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")) if os.path.exists(p)]
    assert found, "the clang++ that hipcc drives (it ships the sanitizers' runtimes) is not under " + rocm
    exe = str(tmp_path / "keytab_pack_check")
    cmd = [found[0], "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", HOST,
           os.path.join(HERE, "keytab_pack_check.cc"), os.path.join(HOST, "aes128.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "keytab pack check: ok"
