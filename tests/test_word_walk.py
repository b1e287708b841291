"""The fused pack kernel steps the buffer descriptor of a wave's next word from the one before (csrc/pg_pair_common.h: PgWordWalk).
That arithmetic is plain C++, so it is walked here without a GPU, window offsets beyond 2^31 and 2^32 bytes included."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_fused_pack_kernels_descriptor_walk_as_a_program_of_its_own(tmp_path):
    """tests/word_walk_main.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: every descriptor of every wave's walk has the
    records and (where it has any) the base of the descriptor worked out from the word's number, and lets through bytes of the
    window's rows only"""
    exe = str(tmp_path / "word_walk_main")
    # (the runtimes linked statically: the program is complete in itself, whatever else the environment loads into a process)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "word_walk_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert r.stdout.decode().strip() == "%d walks, 0 bad" % (4 * 18 * 5 * 28 * 8)
