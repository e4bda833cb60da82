"""The typed kernel call of csrc/pt_call.hpp on the host (tests/call_main.cpp: g++, a recording backend, nothing of HIP): the
right argument list reaches the backend as five slots in order, each the address of the argument's bytes, with the grid, block,
LDS bytes and stream it was given; and each argument list the type rule refuses fails to COMPILE, with the rule's own message.
CPU only."""
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "call_main.cpp")
COUNT = "as many arguments as the kernel has parameters"
TYPES = "every argument of its parameter's type"


def test_the_backend_receives_the_arguments_and_the_launch_shape():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "call_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert out.returncode == 0 and "call: ok" in out.stdout, out.stdout[-2000:]


@pytest.mark.parametrize("bad, message", [(1, TYPES), (2, TYPES), (3, COUNT), (4, TYPES), (5, TYPES), (6, "the kernel's parameter list is not the one")],
                         ids=["int_for_uint32", "float_for_uint32", "one_argument_short", "const_dropped", "foreign_pointee", "handle_of_another_kernel"])
def test_a_wrong_argument_list_does_not_compile(bad, message):
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-DBAD=%d" % bad, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode != 0 and "static assertion failed" in out.stdout and message in out.stdout, out.stdout[-2000:]
