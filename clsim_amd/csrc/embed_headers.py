#!/usr/bin/env python3
"""Writes a file as the initialisers of a byte array (baked_headers.inc: the preprocessed device source the library hands to the
run-time compiler, baked_source.cpp).

    embed_headers.py <input> <output>"""
import sys


def main():
    source, target = sys.argv[1], sys.argv[2]
    with open(source, "rb") as f:
        data = f.read()
    with open(target, "w") as f:
        for i in range(0, len(data), 32):
            f.write(",".join(str(b) for b in data[i:i + 32]) + ",\n")


if __name__ == "__main__":
    main()
