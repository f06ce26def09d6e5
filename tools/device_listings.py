#!/usr/bin/env python3
"""The gfx950 device listings (hipcc -S --cuda-device-only: code + .amdgpu_metadata) of the library's compilations, as
gym-mapf_amd/csrc/Makefile compiles them: its unit table is the list and says the flags, this module only asks make.
Listings are kept under csrc/build/listings (make rebuilds one when its sources change) and read once per process.

    python tools/device_listings.py [name ...]      # builds them, prints name, path and kernel count
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym-mapf_amd', 'csrc')
LISTDIR = os.path.join(CSRC, 'build', 'listings')
_texts = {}


def _make(*args):
    proc = subprocess.run(['make', '--no-print-directory', '-C', CSRC, 'LISTDIR=' + LISTDIR] + list(args),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if proc.returncode:
        raise RuntimeError('make %s failed:\n%s' % (' '.join(args), proc.stderr[-2000:]))
    return proc.stdout


def units():
    """{name: source unit} of the kernel-holding compilations, in the Makefile's order"""
    return dict(line.split() for line in _make('print-kernel-units').splitlines())


def added_units():
    """{name: source unit} of the Makefile's second table: the kernel-holding compilations that entered the library after the first"""
    return dict(line.split() for line in _make('print-added-kernel-units').splitlines())


def joint_units():
    """{name: source unit} of the Makefile's third table: the compilations that follow a joint table policy, whose source lies beside csrc"""
    return dict(line.split() for line in _make('print-joint-kernel-units').splitlines())


def log_units():
    """{name: source unit} of the Makefile's fourth table: the budget compilations that keep an episode log, whose source lies beside csrc"""
    return dict(line.split() for line in _make('print-log-kernel-units').splitlines())


def group_units():
    """{name: source unit} of the Makefile's fifth table: the compilations that follow a group policy, whose source lies beside csrc"""
    return dict(line.split() for line in _make('print-group-kernel-units').splitlines())


def listings(*names):
    """{name: listing text} for the named compilations (a kernel-holding one or a host unit); for all kernel-holding ones if none is named"""
    names = names or tuple(units())
    todo = [n for n in names if n not in _texts]
    if todo:
        _make('-j%d' % min(16, os.cpu_count() or 1), *[os.path.join(LISTDIR, n + '.s') for n in todo])
        for n in todo:
            with open(os.path.join(LISTDIR, n + '.s')) as f:
                _texts[n] = f.read()
    return {n: _texts[n] for n in names}


if __name__ == '__main__':
    import kernel_meta
    for name, text in listings(*sys.argv[1:]).items():
        print('%-28s %s  %d kernels' % (name, os.path.join(LISTDIR, name + '.s'), len(kernel_meta.kernels(text))))
