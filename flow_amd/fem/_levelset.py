# -*- coding: utf-8 -*-
'''
What Distance, Isolines and Regions share on the host: the check of the space,
the check of a field on it, and the loop that sweeps to a fixed point.  The
kernels' common part is csrc/subtri.h.
'''


def scalar_p12_space(V, verb, scalar, name, degree_error=NotImplementedError):
    '''Refuse a space that is not scalar P1 / P2.  verb: what to do on a
    sub-space of a mixed one; scalar: the clause that says the result is
    scalar; name: who takes P1 or P2.'''
    if not hasattr(V, 'layout'):
        raise NotImplementedError(
            'V: a mixed space; %s one of its scalar sub-spaces' % verb)
    if getattr(V, 'component', None) is not None:
        raise NotImplementedError(
            'V: a component view (W.sub(i)); %s: use W.sub(i).collapse()'
            % scalar)
    if V.dim != 1:
        raise NotImplementedError('V: %r components; %s' % (V.dim, scalar))
    if V.degree not in (1, 2):
        raise degree_error('V: P%r; %s takes P1 or P2' % (V.degree, name))


def field_on(V, f, name, built):
    '''f, a Function on V itself (no component view); ValueError otherwise.'''
    from .function import Function
    if not isinstance(f, Function) \
            or getattr(f.function_space(), 'component', None) is not None \
            or not f.function_space().same_as(V):
        raise ValueError('%s: not a Function on the space %s built for'
                         % (name, built))
    return f


def sweep_to_fixed_point(enqueue, a, b, flag, every, limit, what):
    '''Jacobi sweeps from buffer a until a batch's last sweep lowers nothing:
    enqueue(a, b, every) runs `every` sweeps between the two buffers, and one
    integer is read back behind each batch.  (result, other buffer, sweeps);
    _hip.NotConverged after more than `limit` sweeps.'''
    from .. import _hip, device
    sweeps = 0
    while True:
        if sweeps > limit:
            raise _hip.NotConverged(
                '%s: no fixed point after %d sweeps on %d dofs'
                % (what, sweeps, limit))
        flag.zero_()
        enqueue(a, b, every)
        sweeps += every
        if every % 2:
            a, b = b, a
        if int(device.to_host(flag)[0]) == 0:
            return a, b, sweeps
