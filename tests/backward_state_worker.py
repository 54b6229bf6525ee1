"""Worker of tests/test_gpu_backward_state.py::test_shared_layer_with_two_weight_gradient_streams: a fresh process, because
SIDLSG_WGRAD_STREAMS is read when sid_lsg_amd.ops is imported.  Runs the shared-layer cases with two round-robin weight-gradient
streams: the values (the gradient is the sum of both uses), and the ORDER of the two launches on the shared dW as ops.wgrad_order_log
recorded it -- same stream, or a wait_stream of the later launch's stream on the earlier one's before the later launch."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import backward_state_cases as bc  # noqa: E402


def main():
    assert os.environ.get('SIDLSG_WGRAD_STREAMS') == '2', 'run me with SIDLSG_WGRAD_STREAMS=2'
    from sid_lsg_amd import ops
    assert ops.wgrad_stream_count() == 2
    crossed = 0
    for sub in 'abc':
        ops.wgrad_order_log = []
        m = bc.run_shared(sub, f'two streams, shared layer ({sub})')
        dw = next(p for n, p, _ in m.params() if n == 'shared.weight').grad.data_ptr()
        ev = [e for e in ops.wgrad_order_log if e[1] == dw]
        at = [i for i, e in enumerate(ev) if e[0] == 'launch']
        assert len(at) == 2, f'({sub}) expected two launches on the shared dW, got {ev}'
        first, second = ev[at[0]], ev[at[1]]
        waited = any(e[0] == 'wait' and e[2] == second[2] and e[3] == first[2] for e in ev[at[0] + 1:at[1]])
        print(f'({sub}) launches on streams {first[2]:#x}, {second[2]:#x}; wait recorded: {waited}')
        assert first[2] == second[2] or waited, f'({sub}) two launches on one dW on different streams with no wait between them: {ev}'
        crossed += first[2] != second[2]
    assert crossed, 'the round robin never put the two uses on different streams: the cases prove nothing'
    ops.wgrad_order_log = None
    torch.cuda.synchronize()
    print('shared dW ordered on two streams: ok')


if __name__ == '__main__':
    main()
