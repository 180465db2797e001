#!/usr/bin/env python3
"""The cross-pseudo-supervision baseline on MI355X under the reference's file name (``trian_CPS.py``, spelling kept)
and flags: ``train.py --method cps``.  Every flag of train.py is taken (the two reference scripts share theirs);
``--thr``, ``--alpha``, ``--queue-batch`` and ``--temperature`` are accepted and, as in the reference's script, unused."""
import train

if __name__ == '__main__':
    parser = train.build_parser()
    parser.set_defaults(method='cps')
    train.main(parser.parse_args())
