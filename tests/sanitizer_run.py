"""Starting a program built with -fsanitize=thread or -fsanitize=address.  The sanitizer runtimes of GCC 11 expect the kernel to randomise
mmap addresses with at most 28 bits; where it uses more, ThreadSanitizer stops with "unexpected memory mapping" and AddressSanitizer can
loop on DEADLYSIGNAL.  The program is therefore started with address randomisation off for that process alone (`setarch -R`, a
personality flag of the child) wherever that is permitted, which leaves what the sanitizers check unchanged."""
import platform
import shutil
import subprocess


def sanitized(argv):
    setarch = shutil.which("setarch")
    if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        return [setarch, platform.machine(), "-R", *argv]
    return list(argv)
